"""sparse.Rulebook declares its derived state: nothing can be hung on it under another name.  Host code only."""
import dataclasses

import pytest
import torch

from findnpropagate_amd import sparse as S

DERIVED = ("_tile_rb", "_lean", "_marked_next", "_rowmask", "_sorted", "_perm_f32", "_ell", "_no_tile", "_pairs", "_nbr_t", "_in_side")


def _rulebook():
    geom, _ = S.make_geom(3, 1, 1, [8, 8, 8], [8, 8, 8])
    return S.Rulebook(nbr=torch.empty((27, 4), dtype=torch.int32), K=27, cap_out=4, geom=geom)


def test_undeclared_attribute_raises():
    rb = _rulebook()
    for name in ("_sortd", "_tile_rulebook", "_notile", "anything"):     # (a misspelt field used to fall back to the plain kernel)
        with pytest.raises(AttributeError):
            setattr(rb, name, 1)
    with pytest.raises(AttributeError):
        rb._sortd
    assert not hasattr(rb, "__dict__")


def test_fresh_rulebook_has_no_derived_state():
    rb = _rulebook()
    fields = {f.name: f for f in dataclasses.fields(S.Rulebook)}
    assert [n for n in fields if n.startswith("_")] == list(DERIVED)
    for name in DERIVED:
        assert getattr(rb, name) is None, name
        assert not fields[name].init and not fields[name].repr
    with pytest.raises(TypeError):
        S.Rulebook(nbr=rb.nbr, K=27, cap_out=4, geom=rb.geom, _sorted=())     # (derived state is written by its kernel's wrapper only)
    rb._sorted = (rb.nbr, rb.nbr)                                              # the declared names are assignable
    assert _rulebook()._sorted is None
