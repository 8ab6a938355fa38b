"""fnp_sparse_to_dense_backward (the adjoint of the dense map) refuses what it cannot run before it launches anything: host-only,
no GPU needed."""
from findnpropagate_amd import lib


def test_backward_entry_point_rejects_bad_arguments():
    L = lib.load()
    fake = 256   # (never dereferenced: every call below is refused before a launch)
    ok = dict(g=fake, dt=lib.FNP_BF16, co=fake, n=fake, cap=10, C=8, B=1, D=2, H=4, W=4, gf=fake)
    call = lambda a: L.fnp_sparse_to_dense_backward(a["g"], a["dt"], a["co"], a["n"], a["cap"], a["C"], a["B"], a["D"], a["H"], a["W"],
                                                    a["gf"], None, 0, None)
    for key, bad in (("g", None), ("co", None), ("n", None), ("gf", None), ("cap", 0), ("C", 0), ("B", 0), ("D", -1), ("H", 0),
                     ("W", 0), ("dt", 7)):
        assert call(dict(ok, **{key: bad})) == -1, key
