"""FusedResBackbone._plan: the decisions of one forward — which rulebook form, which kernel family, which sorts, which counters —
as the records the index chain and the convolutions consume.  Host code only: no GPU, nothing launched.

The launch trace (test_launch_trace.py) sees a decision only through the launches it causes; here each one is held by itself, so
a flag that flips while the launch list happens to stay the same still fails.  The expected records are written out below from
the conditions of the engine as they stood before the forward was split into phases (VoxelResBackBone8x: conv_input 5 -> 16,
strided layers 16 -> 32, 32 -> 64, 64 -> 128, all 3x3x3; capacities cap1 x (1, 3, 2, 1, 1)):

  16-bit engines   stage 1 on records, and every 16-channel layer with it, unless rulebooks are logged or FNP_ELL forbids;
                   16 -> 32 on records with them; 32 -> 64 and 64 -> 128 resolve their neighbours in the kernel unless logged;
                   stages 2, 3 tiled (lean table and escape counter unless logged) unless FNP_TILE forbids or the gate holds the
                   stage off; stage 4 class-sorted from 131,072 rows of capacity on
  fp32             tables only; every stage class-sorted (f32 sort) from 32,768 rows of capacity on, unless logged
  bf16x3           the SubM stages as the bf16 engine's (its cross terms run on those kernels), the strided layers on tables,
                   no f32 sort
"""
import pytest

import launch_trace as LT
from findnpropagate_amd import sparse as S
from findnpropagate_amd.backbones_3d import spconv_backbone as SB

FIELDS = ("fused", "ell_down", "ch", "tiled", "lean", "srt", "srt32", "esc", "no_tile")


def st(ch, **on):
    """a stage record: `ch` channels, the named flags set, every other one clear"""
    assert set(on) <= set(FIELDS) and all(v in (True, False) for v in on.values())
    return tuple(ch if f == "ch" else on.get(f, False) for f in FIELDS)


def expected(family, big, variant):
    """((ell, ell_all, srt1), [stage 2, stage 3, stage 4]); big: cap1 = 131,072 (else 3,000)"""
    tiled = dict(tiled=True, lean=True, esc=True)
    if family == "half":
        on_records = (True, True, False)
        return {
            "default": (on_records, [st(32, ell_down=True, **tiled), st(64, fused=True, **tiled), st(128, fused=True, srt=big)]),
            "tile_off": (on_records, [st(32, ell_down=True, no_tile=True), st(64, fused=True, **tiled), st(128, fused=True, srt=big)]),
            "rulebook_log": ((False, False, False), [st(32, tiled=True), st(64, tiled=True), st(128, srt=big)]),
            "ELL_MODE=False": ((False, False, False), [st(32, **tiled), st(64, fused=True, **tiled), st(128, fused=True, srt=big)]),
            "ELL_MODE=True ELL_MFMA=False": (on_records, [st(32, ell_down=True, **tiled), st(64, fused=True, **tiled), st(128, fused=True, srt=big)]),
            "TILE_MODE=False": (on_records, [st(32, ell_down=True), st(64, fused=True), st(128, fused=True, srt=big)]),
        }[variant]
    if family == "fp32":
        if variant == "rulebook_log":
            return (False, False, False), [st(32), st(64), st(128)]
        return (False, False, big), [st(32, srt32=big, no_tile=variant == "tile_off"), st(64, srt32=big), st(128, srt32=big)]
    assert family == "bf16x3"
    return (False, False, False), {
        "default": [st(32, **tiled), st(64, **tiled), st(128, srt=big)],
        "tile_off": [st(32, no_tile=True), st(64, **tiled), st(128, srt=big)],
        "rulebook_log": [st(32, tiled=True), st(64, tiled=True), st(128, srt=big)],
        "ELL_MODE=False": [st(32, **tiled), st(64, **tiled), st(128, srt=big)],
        "ELL_MODE=True ELL_MFMA=False": [st(32, **tiled), st(64, **tiled), st(128, srt=big)],
        "TILE_MODE=False": [st(32), st(64), st(128, srt=big)],
    }[variant]


@pytest.fixture(scope="module")
def modules():
    return {d: SB.VoxelResBackBone8x({"USE_BIAS": False, "FNP_DTYPE": d}, 5, [64, 64, 8]).eval() for d in ("bf16", "fp16", "fp32", "bf16x3")}


@pytest.mark.parametrize("variant", LT.ENGINE_VARIANTS)
@pytest.mark.parametrize("cap1", [3000, 131072])
@pytest.mark.parametrize("fnp_dtype", ["bf16", "fp16", "fp32", "bf16x3"])
def test_plan_records(modules, monkeypatch, fnp_dtype, cap1, variant):
    eng = SB.FusedResBackbone(modules[fnp_dtype])
    switches = {"TILE_MODE": None, "ELL_MODE": None, "ELL_MFMA": True}
    if variant == "tile_off":
        eng.tile_off = {0: 5}
    elif variant == "rulebook_log":
        eng.rulebook_log = []
    elif variant == "ELL_MODE=False":
        switches["ELL_MODE"] = False
    elif variant == "ELL_MODE=True ELL_MFMA=False":
        switches["ELL_MODE"], switches["ELL_MFMA"] = True, False
    elif variant == "TILE_MODE=False":
        switches["TILE_MODE"] = False
    else:
        assert variant == "default"
    for name, value in switches.items():
        monkeypatch.setattr(S, name, value)
    caps = [cap1, 3 * cap1, 2 * cap1, cap1, cap1]
    assert [cap1] + [max(256, int(cap1 * f)) for f in eng.cap_factor] == caps
    plan1, stages = eng._plan(eng.prepare(), caps)
    family = "half" if fnp_dtype in ("bf16", "fp16") else fnp_dtype
    want1, want = expected(family, cap1 == 131072, variant)
    assert tuple(plan1) == want1 and plan1._fields == ("ell", "ell_all", "srt1")
    assert [s._fields for s in stages] == [FIELDS] * 3
    assert [tuple(s) for s in stages] == want
    assert all(type(v) is bool for v in plan1) and all(type(v) is (int if f == "ch" else bool) for s in stages for f, v in zip(FIELDS, s))
