"""The host layer's kernel choices, held to tests/golden/launch_trace.json (see tests/launch_trace.py).  No GPU.

Every forward kernel gives the plain kernel's bits, so only the trace shows which one a call takes: conv_forward and
conv_forward_split over their arguments and the rulebook's derived state, the 32-bit-offset fall-backs, conv_forward_ell, the
kernels the backward of SparseConvFunction picks, and the whole launch list of FusedResBackbone.run for every engine dtype —
eager, and in the four forms a _PointsGraph captures it (one or two graphs, the index chain a graph of its own or not).
The comparison is exact: same entry points, same arguments, same order."""
import pytest

import launch_trace as LT


@pytest.fixture(scope="module")
def golden():
    return LT.load()


@pytest.mark.parametrize("section", list(LT.SECTIONS))
def test_trace_equals_fixture(golden, section):
    want = golden["sections"][section]
    ids, traces = LT.record(section)
    assert len(ids) == want["cases"] and LT._ids_digest(ids) == want["ids_sha256"], "the case list differs from the fixture's"
    assert want.get("ids", ids) == ids
    table = golden["calls"]
    for cid, calls, numbers in zip(ids, traces, want["calls_of_case"]):
        assert calls == [table[i] for i in numbers], cid


def test_fixture_covers_every_route(golden):
    """(the fixture itself: each kernel of the forward chains, the refusal and every fall-back is met by some case)"""
    names = {c[0] for c in golden["calls"]}
    assert {"fnp_spconv_forward", "fnp_spconv_forward_tiled", "fnp_spconv_forward_sorted", "fnp_spconv_forward_f32_sorted",
            "fnp_spconv_forward_split", "fnp_spconv_forward_tiled_split", "fnp_spconv_forward_sorted_split", "fnp_tile_rulebook_build",
            "fnp_spconv_forward_ell", "fnp_spconv_forward_ell_mfma", "fnp_spconv_forward_strided", "fnp_rulebook_transpose",
            "fnp_rulebook_pairs", "fnp_spconv_wgrad_pairs", "fnp_spconv_wgrad", "fnp_rulebook_classsort", "fnp_rulebook_classsort_f32",
            "fnp_rulebook_subm_tiled_lean", "fnp_rulebook_subm_masked", "fnp_rulebook_ell", "raise"} <= names
    table, limits = golden["calls"], golden["sections"]["limits"]
    plain = ("fnp_spconv_forward", "fnp_spconv_forward_split")
    for i, (cid, numbers) in enumerate(zip(limits["ids"], limits["calls_of_case"])):
        call = table[numbers[0]]
        at_limit = i % 2 == 1             # (the cases come in pairs: one row below the limit, then at it)
        if cid.startswith("permuted weight"):
            assert call[0] == "fnp_spconv_forward" and call[4][2] == (not at_limit), cid     # (the weight: un-permuted at the limit)
        else:
            assert (call[0] in plain) == at_limit, cid
