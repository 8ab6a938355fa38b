"""What the convolution forward entry points refuse, and what they let through, as a table of calls into the built library.

No GPU: every address is a fake (never dereferenced by host code), a refused call returns FNP_ERR_ARG (-1) before any HIP call,
and a call that passes validation goes on to a launch that fails for want of a device (FNP_ERR_LAUNCH or FNP_ERR_HIP).  So both
sides of every boundary show without a device.  With a device present the fake addresses would reach a kernel: the module skips
itself then."""
import ctypes

import pytest
import torch

from findnpropagate_amd import lib as _l

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake addresses must never reach a launch: CPU-only test")

F32, BF16, F16, NO_DTYPE = _l.FNP_F32, _l.FNP_BF16, _l.FNP_F16, 7
HINT_W_PERMUTED = 4
ERR_ARG, ERR_WORKSPACE = -1, -4
LIMIT = 0x7FFFFFFF   # first byte count the 32-bit buffer offsets refuse

# fake device addresses, 64 KiB apart (so +4 / +8 break exactly the alignment they are meant to break)
X, W, NBR, NOUT, Y, SCALE, SHIFT, RES, PERM, BMASK, TRB, REC, ADD, HI, LO, COORDS, RMASK, WS = (0x10000 * (i + 1) for i in range(18))

_GRID = _l.RankGridC(2, 11, 60, 61, 0x200000, 0x210000, 0x220000, None, None)
_GEOM = _l.ConvGeom((3, 3, 3), (2, 2, 2), (1, 1, 1), (11, 60, 61), (6, 30, 31))


def _grid(**kw):
    g = _l.RankGridC(_GRID.B, _GRID.D, _GRID.H, _GRID.W, _GRID.bits, _GRID.base, _GRID.summary, None, None)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _geom(field, axis, value):
    g = _l.ConvGeom(tuple(_GEOM.ksize), tuple(_GEOM.stride), tuple(_GEOM.padding), tuple(_GEOM.in_shape), tuple(_GEOM.out_shape))
    getattr(g, field)[axis] = value
    return g


# entry -> its arguments in ABI order with the values of one plain accepted call
ENTRIES = {
    "fnp_spconv_forward": dict(feat_in=X, in_dtype=BF16, n_in_rows=1000, weight=W, nbr=NBR, nbr_stride=1024, K=27, n_out=NOUT, cap_out=1024,
                               feat_out=Y, out_dtype=BF16, scale=None, shift=None, residual=None, relu=0, hints=0, Cin=32, Cout=32, stream=None),
    "fnp_spconv_forward_split": dict(feat_in=X, in_dtype=BF16, n_in_rows=1000, weight=W, nbr=NBR, nbr_stride=1024, K=27, n_out=NOUT, cap_out=1024,
                                     feat_out=Y, scale=None, shift=None, residual=None, addend=None, relu=0, hints=0, Cin=32, Cout=32,
                                     out_hi=HI, out_lo=LO, stream=None),
    "fnp_spconv_forward_strided": dict(feat_in=X, in_dtype=BF16, n_in_rows=1000, weight=W, in_grid=_GRID, geom=_GEOM, out_coords=COORDS,
                                       n_out=NOUT, cap_out=1024, feat_out=Y, out_dtype=BF16, scale=None, shift=None, relu=0, Cin=16, Cout=32,
                                       stream=None),
    "fnp_spconv_forward_ell": dict(feat_in=X, in_dtype=BF16, n_in_rows=1000, weight=W, records=REC, cap_rows=1024, pool_records=256, n_out=NOUT,
                                   feat_out=Y, out_dtype=BF16, scale=None, shift=None, residual=None, relu=0, Cin=16, Cout=16, stream=None),
    "fnp_spconv_forward_ell_mfma": dict(feat_in=X, in_dtype=BF16, n_in_rows=1000, weight=W, records=REC, cap_rows=1024, pool_records=256,
                                        n_out=NOUT, feat_out=Y, out_dtype=BF16, scale=None, shift=None, residual=None, relu=0, Cin=16, Cout=16,
                                        stream=None),
    "fnp_spconv_forward_sorted": dict(feat_in=X, dtype=BF16, n_in_rows=1000, weight=W, nbr=NBR, nbr_stride=1024, perm=PERM, blockmask=BMASK,
                                      n_out=NOUT, cap_out=1024, feat_out=Y, scale=None, shift=None, residual=None, relu=0, Cin=128, Cout=128,
                                      stream=None),
    "fnp_spconv_forward_sorted_split": dict(feat_in=X, dtype=BF16, n_in_rows=1000, weight=W, nbr=NBR, nbr_stride=1024, perm=PERM, blockmask=BMASK,
                                            n_out=NOUT, cap_out=1024, feat_out=Y, scale=None, shift=None, residual=None, addend=None, relu=0,
                                            Cin=128, Cout=128, out_hi=HI, out_lo=LO, stream=None),
    "fnp_spconv_forward_f32_sorted": dict(feat_in=X, n_in_rows=1000, weight=W, nbr=NBR, nbr_stride=1024, perm=PERM, n_out=NOUT, cap_out=1024,
                                          feat_out=Y, scale=None, shift=None, residual=None, relu=0, wperm=0, Cin=64, Cout=64, stream=None),
    "fnp_spconv_forward_tiled": dict(feat_in=X, dtype=BF16, n_in_rows=1000, weight=W, tile_rb=TRB, nbr=NBR, nbr_stride=1024, n_out=NOUT,
                                     cap_out=1024, feat_out=Y, scale=None, shift=None, residual=None, relu=0, Cin=32, Cout=32, stream=None),
    "fnp_spconv_forward_tiled_split": dict(feat_in=X, dtype=BF16, n_in_rows=1000, weight=W, tile_rb=TRB, nbr=NBR, nbr_stride=1024, n_out=NOUT,
                                           cap_out=1024, feat_out=Y, scale=None, shift=None, residual=None, addend=None, relu=0, Cin=32, Cout=32,
                                           out_hi=HI, out_lo=LO, stream=None),
    "fnp_rulebook_classsort": dict(nbr=NBR, nbr_stride=1024, K=27, rowmask=RMASK, n_out=NOUT, cap_out=1024, Cin=128, Cout=128, perm=PERM,
                                   blockmask=BMASK, workspace=WS, workspace_bytes=4096, stream=None),
    "fnp_rulebook_classsort_f32": dict(rowmask=RMASK, n_out=NOUT, cap_out=1024, Cin=64, Cout=64, perm=PERM, stream=None),
}

REFUSED, PASSES = "refused", "passes"

# (entry, overrides of the accepted call, outcome)
TABLE = []


def _add(entry, outcome, **kw):
    assert set(kw) <= set(ENTRIES[entry]), (entry, kw)
    TABLE.append((entry, kw, outcome))


def _common(entry, required, dtype_fields=()):
    """The refusals every forward entry shares, where the entry has the argument (dtype_fields: its 16-bit type codes)."""
    base = ENTRIES[entry]
    _add(entry, PASSES)   # the plain accepted call
    for p in required:
        _add(entry, REFUSED, **{p: None})
    cap = "cap_out" if "cap_out" in base else "cap_rows"
    _add(entry, REFUSED, **{cap: 0})
    if "nbr_stride" in base and "rowmask" not in base:   # (the class sort reads the table only without row masks)
        _add(entry, REFUSED, nbr_stride=base[cap] - 1)
        _add(entry, PASSES, nbr_stride=base[cap])
    if "n_in_rows" in base:
        _add(entry, REFUSED, n_in_rows=0)
        _add(entry, PASSES, n_in_rows=1)
    if "scale" in base:
        _add(entry, REFUSED, scale=SCALE)
        _add(entry, REFUSED, shift=SHIFT)
        _add(entry, PASSES, scale=SCALE, shift=SHIFT)
    if dtype_fields:
        _add(entry, REFUSED, **{dtype_fields[0]: NO_DTYPE})
        _add(entry, PASSES, **{f: F16 for f in dtype_fields})


# ---- fnp_spconv_forward: any channel pair runs (thread-per-element kernel), features beyond 32-bit offsets too
E = "fnp_spconv_forward"
_common(E, ["feat_in", "weight", "nbr", "n_out", "feat_out"])
_add(E, REFUSED, K=0)
_add(E, REFUSED, Cin=0)
_add(E, REFUSED, Cout=0)
_add(E, REFUSED, in_dtype=NO_DTYPE)
_add(E, REFUSED, out_dtype=NO_DTYPE)
_add(E, REFUSED, in_dtype=BF16, out_dtype=F16)
_add(E, REFUSED, in_dtype=F16, out_dtype=BF16)
_add(E, PASSES, in_dtype=F16, out_dtype=F16)
_add(E, PASSES, in_dtype=BF16, out_dtype=F32)
_add(E, PASSES, in_dtype=F16, out_dtype=F32)
_add(E, PASSES, Cin=48, Cout=48)
_add(E, PASSES, n_in_rows=(1 << 25) - 1)             # 32 ch x 2 bytes: one row below the limit (matrix kernel)
_add(E, PASSES, n_in_rows=1 << 25)                   # at it (thread-per-element kernel: 64-bit addresses)
_add(E, PASSES, K=3, Cin=128, Cout=128, cap_out=256 * 8 * 64, nbr_stride=256 * 8 * 64)   # conv_out's own kernel
_add(E, PASSES, in_dtype=F32, out_dtype=F32)
_add(E, PASSES, in_dtype=F32, out_dtype=BF16)
_add(E, PASSES, in_dtype=F32, out_dtype=F16)
_add(E, REFUSED, in_dtype=F32, out_dtype=NO_DTYPE)
_add(E, PASSES, in_dtype=F32, out_dtype=F32, Cin=4, Cout=16)     # the first layer's kernel
_add(E, PASSES, in_dtype=F32, out_dtype=F16, Cin=4, Cout=16)
_add(E, REFUSED, in_dtype=F32, out_dtype=NO_DTYPE, Cin=4, Cout=16)
_add(E, PASSES, in_dtype=F32, out_dtype=F32, hints=HINT_W_PERMUTED)
_add(E, REFUSED, in_dtype=F32, out_dtype=F32, hints=HINT_W_PERMUTED, Cin=48, Cout=48)   # a shape the f32 matrix kernel lacks
_add(E, REFUSED, in_dtype=F32, out_dtype=BF16, hints=HINT_W_PERMUTED)
_add(E, PASSES, in_dtype=F32, out_dtype=F32, hints=HINT_W_PERMUTED, n_in_rows=(1 << 24) - 1)   # 32 ch x 4 bytes below the limit
_add(E, REFUSED, in_dtype=F32, out_dtype=F32, hints=HINT_W_PERMUTED, n_in_rows=1 << 24)
_add(E, PASSES, in_dtype=F32, out_dtype=F32, n_in_rows=1 << 24)

# ---- fnp_spconv_forward_split: the matrix kernel only
E = "fnp_spconv_forward_split"
_common(E, ["feat_in", "weight", "nbr", "n_out", "out_hi", "out_lo"], ("in_dtype",))
_add(E, PASSES, feat_out=None)
_add(E, REFUSED, K=0)
_add(E, REFUSED, Cin=0)
_add(E, REFUSED, in_dtype=F32)
_add(E, REFUSED, Cin=48, Cout=48)
_add(E, PASSES, Cin=64, Cout=128)
_add(E, PASSES, n_in_rows=(1 << 25) - 1)
_add(E, REFUSED, n_in_rows=1 << 25)
for p, a in (("out_hi", HI), ("out_lo", LO), ("addend", ADD)):
    _add(E, REFUSED, **{p: a + 4})
    _add(E, PASSES, **{p: a + 8})
_add(E, REFUSED, feat_out=Y + 8)
_add(E, PASSES, feat_out=Y + 16)

# ---- fnp_spconv_forward_strided
E = "fnp_spconv_forward_strided"
_common(E, ["feat_in", "weight", "in_grid", "geom", "out_coords", "n_out", "feat_out"], ("in_dtype", "out_dtype"))
_add(E, REFUSED, in_dtype=F16)                        # out_dtype stays bf16
_add(E, REFUSED, in_dtype=F32, out_dtype=F32)
_add(E, REFUSED, out_dtype=F32)
_add(E, REFUSED, in_grid=_grid(bits=None))
_add(E, REFUSED, in_grid=_grid(B=0))
_add(E, REFUSED, in_grid=_grid(D=12))                 # not the geometry's input shape
_add(E, REFUSED, geom=_geom("ksize", 1, 2))
_add(E, REFUSED, geom=_geom("stride", 2, 0))
_add(E, REFUSED, geom=_geom("padding", 0, -1))
_add(E, PASSES, geom=_geom("padding", 0, 0))
_add(E, REFUSED, Cin=16, Cout=16)
_add(E, REFUSED, Cin=32, Cout=32)
_add(E, PASSES, Cin=32, Cout=64)
_add(E, PASSES, Cin=64, Cout=128)
_add(E, PASSES, n_in_rows=(1 << 26) - 1)             # 16 ch x 2 bytes
_add(E, REFUSED, n_in_rows=1 << 26)

# ---- fnp_spconv_forward_ell (records: no alignment check) and fnp_spconv_forward_ell_mfma (16-byte records)
for E in ("fnp_spconv_forward_ell", "fnp_spconv_forward_ell_mfma"):
    _common(E, ["feat_in", "weight", "records", "n_out", "feat_out"], ("in_dtype", "out_dtype"))
    _add(E, REFUSED, in_dtype=F16)
    _add(E, REFUSED, out_dtype=F32)
    _add(E, REFUSED, pool_records=-1)
    _add(E, PASSES, pool_records=0)
    _add(E, PASSES, pool_records=(1 << 26) - 1024 - 1)
    _add(E, REFUSED, pool_records=(1 << 26) - 1024)
    _add(E, REFUSED, Cin=32, Cout=32)
    _add(E, REFUSED, Cout=48)
    _add(E, REFUSED, Cout=64)
    _add(E, PASSES, Cout=32)
    _add(E, PASSES, n_in_rows=(1 << 26) - 1)
    _add(E, REFUSED, n_in_rows=1 << 26)
    _add(E, PASSES, residual=RES)
_add("fnp_spconv_forward_ell", PASSES, records=REC + 4)
_add("fnp_spconv_forward_ell_mfma", REFUSED, records=REC + 8)
_add("fnp_spconv_forward_ell_mfma", PASSES, records=REC + 16)
_add("fnp_spconv_forward_ell_mfma", REFUSED, in_dtype=F32, out_dtype=F32, Cin=4)
E = "fnp_spconv_forward_ell"   # its f32 first layer: 4 or 5 point features -> 16 channels of any type
for out in (F32, BF16, F16):
    _add(E, PASSES, in_dtype=F32, out_dtype=out, Cin=4)
_add(E, PASSES, in_dtype=F32, out_dtype=F32, Cin=5)
_add(E, REFUSED, in_dtype=F32, out_dtype=NO_DTYPE, Cin=4)
_add(E, REFUSED, in_dtype=F32, out_dtype=F32, Cin=6)
_add(E, REFUSED, in_dtype=F32, out_dtype=F32, Cin=4, Cout=32)
_add(E, PASSES, in_dtype=F32, out_dtype=F32, Cin=4, n_in_rows=(1 << 27) - 1)
_add(E, REFUSED, in_dtype=F32, out_dtype=F32, Cin=4, n_in_rows=1 << 27)

# ---- fnp_spconv_forward_sorted / _sorted_split: 128 -> 128 only; 32768 rows and more take the row pipeline
for E in ("fnp_spconv_forward_sorted", "fnp_spconv_forward_sorted_split"):
    split = E.endswith("_split")
    _common(E, ["feat_in", "weight", "nbr", "perm", "blockmask", "n_out"] + (["out_hi", "out_lo"] if split else ["feat_out"]), ("dtype",))
    _add(E, REFUSED, dtype=F32)
    _add(E, REFUSED, Cin=64, Cout=64)
    _add(E, REFUSED, Cin=64)
    _add(E, REFUSED, Cout=64)
    _add(E, PASSES, n_in_rows=(1 << 23) - 1)         # 128 ch x 2 bytes
    _add(E, REFUSED, n_in_rows=1 << 23)
    for cap in (256 * 8 * 16 - 1, 256 * 8 * 16):
        _add(E, PASSES, cap_out=cap, nbr_stride=cap)
        _add(E, PASSES, cap_out=cap, nbr_stride=cap, dtype=F16)
        _add(E, REFUSED, cap_out=cap, nbr_stride=cap, dtype=NO_DTYPE)
        _add(E, REFUSED, cap_out=cap, nbr_stride=cap, n_in_rows=1 << 23)
    _add(E, PASSES, residual=RES)
E = "fnp_spconv_forward_sorted_split"
_add(E, PASSES, feat_out=None)
for p, a in (("out_hi", HI), ("out_lo", LO), ("addend", ADD)):
    _add(E, REFUSED, **{p: a + 4})
    _add(E, PASSES, **{p: a + 8})
_add(E, REFUSED, feat_out=Y + 8)
_add(E, PASSES, feat_out=Y + 16)

# ---- fnp_spconv_forward_f32_sorted: Cin == Cout in {16, 32, 64, 128}
E = "fnp_spconv_forward_f32_sorted"
_common(E, ["feat_in", "weight", "nbr", "perm", "n_out", "feat_out"])
for c in (16, 32, 128):
    _add(E, PASSES, Cin=c, Cout=c)
_add(E, PASSES, wperm=1)
_add(E, REFUSED, Cin=48, Cout=48)
_add(E, REFUSED, Cin=32, Cout=64)
_add(E, REFUSED, Cin=8, Cout=8)
_add(E, PASSES, n_in_rows=(1 << 23) - 1)             # 64 ch x 4 bytes
_add(E, REFUSED, n_in_rows=1 << 23)

# ---- fnp_spconv_forward_tiled / _tiled_split: 32 -> 32 and 64 -> 64, everything 16-byte aligned
for E in ("fnp_spconv_forward_tiled", "fnp_spconv_forward_tiled_split"):
    split = E.endswith("_split")
    _common(E, ["feat_in", "weight", "tile_rb", "nbr", "n_out"] + (["out_hi", "out_lo"] if split else ["feat_out"]), ("dtype",))
    _add(E, REFUSED, dtype=F32)
    _add(E, REFUSED, Cin=16, Cout=16)
    _add(E, REFUSED, Cin=32, Cout=64)
    _add(E, REFUSED, Cin=128, Cout=128)
    _add(E, PASSES, Cin=64, Cout=64)
    _add(E, PASSES, Cin=64, Cout=64, dtype=F16)
    _add(E, PASSES, n_in_rows=(1 << 25) - 1)
    _add(E, REFUSED, n_in_rows=1 << 25)
    _add(E, PASSES, nbr_stride=(LIMIT - 1) // 108)   # the int32 table: 27 x stride x 4 bytes
    _add(E, REFUSED, nbr_stride=(LIMIT - 1) // 108 + 1)
    for p, a in (("tile_rb", TRB), ("feat_in", X), ("feat_out", Y), ("weight", W), ("residual", RES)):
        _add(E, REFUSED, **{p: a + 8})
        _add(E, PASSES, **{p: a + 16})
E = "fnp_spconv_forward_tiled_split"
_add(E, PASSES, feat_out=None)
for p, a in (("out_hi", HI), ("out_lo", LO), ("addend", ADD)):
    _add(E, REFUSED, **{p: a + 4})
    _add(E, PASSES, **{p: a + 8})

# ---- the class sorts
E = "fnp_rulebook_classsort"
_common(E, ["n_out", "perm", "blockmask"])
_add(E, REFUSED, K=26)
_add(E, REFUSED, Cin=64, Cout=64)
_add(E, REFUSED, Cin=64)
_add(E, REFUSED, Cout=64)
_add(E, PASSES, nbr=None, workspace=None, workspace_bytes=0, nbr_stride=0)   # with row masks the table is not read
_add(E, PASSES, rowmask=None)
_add(E, REFUSED, rowmask=None, nbr=None)
_add(E, REFUSED, rowmask=None, nbr_stride=1023)
_add(E, REFUSED, rowmask=None, workspace=None)
_add(E, ERR_WORKSPACE, rowmask=None, workspace_bytes=4095)
E = "fnp_rulebook_classsort_f32"
_common(E, ["rowmask", "n_out", "perm"])
for c in (16, 32, 128):
    _add(E, PASSES, Cin=c, Cout=c)
_add(E, REFUSED, Cin=48, Cout=48)
_add(E, REFUSED, Cin=16, Cout=32)


def _call(L, entry, overrides):
    args = dict(ENTRIES[entry], **overrides)
    vals = [ctypes.byref(v) if isinstance(v, ctypes.Structure) else v for v in args.values()]
    return getattr(L, entry)(*vals)


def test_the_table_covers_every_entry_on_both_sides():
    for entry in ENTRIES:
        outcomes = {o for e, _, o in TABLE if e == entry}
        assert REFUSED in outcomes and PASSES in outcomes, entry
    assert len(ENTRIES) == 12


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_refuses_and_accepts_what_it_did(entry):
    L = _l.load()
    bad = []
    for e, kw, outcome in TABLE:
        if e != entry:
            continue
        rc = _call(L, e, kw)
        if outcome == REFUSED:
            ok = rc == ERR_ARG
        elif outcome == PASSES:
            # only "not refused": what a launch without a device returns (FNP_ERR_LAUNCH, or FNP_ERR_HIP where the LDS limit is
            # raised first) is the runtime's business, not the contract's
            ok = rc != ERR_ARG
        else:
            ok = rc == outcome
        if not ok:
            bad.append((kw, outcome, rc))
    assert not bad, bad
