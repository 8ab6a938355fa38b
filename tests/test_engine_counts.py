"""FusedResBackbone._digest_counts: what the host does with the counts a forward reads back — the one path behind the eager
forward, the graphed forward and PointsPipeline.result.  Host code only: no GPU, no library.  The lists are written by hand in
the order the counts launch stores them (five stage counts, the tiled kernels' time-out word, then the engine's counters in
the order of `ell_used`); the expected numbers are worked out here from the growth and gate rules, not taken from the engine."""
import pytest

from findnpropagate_amd import lib
from findnpropagate_amd.backbones_3d import spconv_backbone as SB

CAP1 = 2000
CAPS = [CAP1, 6000, 4000, 2000, 2000]                 # cap1 x (1, 3.0, 2.0, 1.0, 1.0): the engine's initial cap_factor
POOL1, POOL2 = int(CAP1 * 0.25) + 64, int(CAPS[1] * 0.0625) + 64     # the record pools the initial ell_pool gives: 564, 439
# (counter tensor — unused on the host —, pool size, which): stage-1 records, 16 -> 32 records, escape groups of stages 2 and 3
ELL_USED = [(None, POOL1, 0), (None, POOL2, 1), (None, None, ("esc", 0)), (None, None, ("esc", 1))]
SEEN = 7                                              # the time-out counter as the process last saw it


@pytest.fixture(scope="module")
def module():
    return SB.VoxelResBackBone8x({'USE_BIAS': False}, 5, [64, 64, 8])


@pytest.fixture
def engine(module, monkeypatch):
    monkeypatch.setattr(SB, "_ABORTS_SEEN", SEEN)
    e = SB.FusedResBackbone(module)
    assert e.cap_factor == [3.0, 2.0, 1.0, 1.0] and e.ell_pool == [0.25, 0.0625]
    assert [CAP1] + [max(256, int(CAP1 * f)) for f in e.cap_factor] == CAPS
    return e


def read_back(stages=(1800, 3200, 1500, 800, 700), word=SEEN, used1=100, used2=50, esc2=0, esc3=0):
    return list(stages) + [word, used1, used2, esc2, esc3]


def test_within_capacity_nothing_moves(engine):
    counts = read_back()
    assert engine._digest_counts(counts, ELL_USED, CAPS) is False
    assert counts == [1800, 3200, 1500, 800, 700]
    assert engine.cap_factor == [3.0, 2.0, 1.0, 1.0] and engine.ell_pool == [0.25, 0.0625]
    assert engine.tile_off == {} and engine.tile_period == {}
    assert engine.tile_escape_share == {0: 0.0, 1: 0.0}
    # exactly full is not an overflow
    counts = read_back(stages=CAPS, used1=POOL1, used2=POOL2)
    assert engine._digest_counts(counts, ELL_USED, CAPS) is False
    assert counts == CAPS and engine.cap_factor == [3.0, 2.0, 1.0, 1.0] and engine.ell_pool == [0.25, 0.0625]


@pytest.mark.parametrize("rows, factor", [(10000, 10000 * 1.25 / CAP1),      # far over: 1.25 x what was needed (6.25)
                                          (4001, 2.0 * 2.0)])                # just over: twice the old factor
def test_stage_three_over_capacity_grows_its_factor(engine, rows, factor):
    counts = read_back(stages=(1800, 3200, rows, 800, 700))
    assert engine._digest_counts(counts, ELL_USED, CAPS) is True
    assert counts == [1800, 3200, rows, 800, 700]
    assert engine.cap_factor == [3.0, factor, 1.0, 1.0] and engine.ell_pool == [0.25, 0.0625]


def test_every_stage_over_capacity_grows_every_factor(engine):
    counts = read_back(stages=(1800, 24000, 4001, 8000, 2001))
    assert engine._digest_counts(counts, ELL_USED, CAPS) is True
    assert engine.cap_factor == [24000 * 1.25 / CAP1, 4.0, 8000 * 1.25 / CAP1, 2.0]


@pytest.mark.parametrize("used, factor", [(1600, 1600 * 1.25 / CAP1),        # 1.0
                                          (POOL1 + 1, 2.0 * 0.25)])
def test_stage_one_pool_over_its_size_grows_the_pool(engine, used, factor):
    counts = read_back(used1=used)
    assert engine._digest_counts(counts, ELL_USED, CAPS) is True
    assert counts == [1800, 3200, 1500, 800, 700]
    assert engine.ell_pool == [factor, 0.0625] and engine.cap_factor == [3.0, 2.0, 1.0, 1.0]


def test_strided_layer_pool_is_measured_in_stage_two_rows(engine):
    counts = read_back(used2=1200)
    assert engine._digest_counts(counts, ELL_USED, CAPS) is True
    assert engine.ell_pool == [0.25, 1200 * 1.25 / (CAP1 * 3.0)]     # 0.25 (twice the old factor would be 0.125)


def test_escape_share_closes_the_tile_gate_without_a_rerun(engine):
    E = SB.FusedResBackbone
    groups = 3200 / 32.0                                  # 32-row groups of stage 2
    dense = int(E.TILE_ESC_MAX * groups) + 1              # the first count whose share is above the threshold
    assert dense / groups > E.TILE_ESC_MAX >= (dense - 1) / groups
    counts = read_back(esc2=dense)
    assert engine._digest_counts(counts, ELL_USED, CAPS) is False
    assert counts == [1800, 3200, 1500, 800, 700]
    assert engine.tile_escape_share[0] == dense / groups
    assert engine.tile_off == {0: E.TILE_REPROBE} and engine.tile_period == {0: E.TILE_REPROBE}
    assert engine.cap_factor == [3.0, 2.0, 1.0, 1.0] and engine.ell_pool == [0.25, 0.0625]
    # every re-probe that fails again doubles the period, up to TILE_REPROBE_MAX
    period = E.TILE_REPROBE
    while period < E.TILE_REPROBE_MAX:
        period = min(period * 2, E.TILE_REPROBE_MAX)
        assert engine._digest_counts(read_back(esc2=dense), ELL_USED, CAPS) is False
        assert engine.tile_off == {0: period} and engine.tile_period == {0: period}
    assert engine._digest_counts(read_back(esc2=dense), ELL_USED, CAPS) is False
    assert engine.tile_off == {0: E.TILE_REPROBE_MAX} and engine.tile_period == {0: E.TILE_REPROBE_MAX}
    # a share at or below the threshold forgets the period: the next dense frame starts at TILE_REPROBE again
    assert engine._digest_counts(read_back(esc2=dense - 1), ELL_USED, CAPS) is False
    assert engine.tile_period == {} and engine.tile_escape_share[0] == (dense - 1) / groups
    assert engine._digest_counts(read_back(esc2=dense), ELL_USED, CAPS) is False
    assert engine.tile_off == {0: E.TILE_REPROBE} and engine.tile_period == {0: E.TILE_REPROBE}


def test_time_out_word_raises_once(engine):
    with pytest.raises(lib.FnpError, match="2 hand-over"):
        engine._digest_counts(read_back(word=SEEN + 2), ELL_USED, CAPS)
    assert SB._ABORTS_SEEN == SEEN + 2
    counts = read_back(word=SEEN + 2)
    assert engine._digest_counts(counts, ELL_USED, CAPS) is False          # the same value again: nothing new
    assert counts == [1800, 3200, 1500, 800, 700]
    other = SB.FusedResBackbone(engine.m)                                   # (the counter is the library's, not an engine's)
    assert other._digest_counts(read_back(word=SEEN + 2), ELL_USED, CAPS) is False
