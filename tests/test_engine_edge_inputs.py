"""CPU preconditions of tests/test_gpu_engine_edges.py: what its inputs are
claimed to be, checked with the float64 oracle alone, and that its case table
reaches every dispatch tier of the propagation engine (tier predicates restated
from ggnn_amd/csrc/ggnn_api.hip in tests/engine_edge_cases.py)."""
import numpy as np
import pytest

import engine_edge_cases as EC

FP32_CASES = EC.TIER_CASES + EC.EXTRA_CASES + EC.EMPTY_CASES + EC.PAIR_CASES
DROPOUT_CASES = [c for c in EC.ALL_CASES.values() if EC.dropout_of(c) is not None]


def test_tables_are_tiny():
    for c in EC.ALL_CASES.values():
        assert c.b <= 16 and c.v <= 128, c
        assert c.T <= 3 or c.name == "fused_maxt", c
    assert EC.ALL_CASES["fused_maxt"].T == EC.FUSED_MAXT
    assert set(EC.DENSE_CHANNEL_CASES) <= {c.name for c in EC.TIER_CASES}


@pytest.mark.parametrize("name", [c.name for c in EC.EMPTY_CASES])
def test_empty_graph_and_channel_really_are_empty(name):
    c = EC.ALL_CASES[name]
    A = EC.inputs(name)["A"]
    assert not A[0].any()                      # graph 0 has no edge
    assert not A[:, c.C - 1].any()             # the last channel has no edge in any graph
    for ch in range(c.C - 1):                  # every other channel has one somewhere
        assert A[:, ch].any(), ch
    for g in range(1, c.b):                    # and every other graph has edges
        assert A[g].any(), g
    _, gref, _ = EC.reference(name)
    assert not gref["edge_weights"][c.C - 1].any()     # exactly 0 in the oracle
    assert not gref["edge_biases"][c.C - 1].any()
    assert gref["edge_weights"][:c.C - 1].any() and gref["edge_biases"][:c.C - 1].any()


@pytest.mark.parametrize("name", [c.name for c in DROPOUT_CASES])
def test_dropout_cases_move_the_oracle(name):
    """"Dropout is really on": the same step without it differs by > 0.05."""
    ref, _, nodrop = EC.reference(name)
    assert nodrop is not None
    assert np.abs(nodrop - ref).max() > 0.05


@pytest.mark.parametrize("name", [c.name for c in FP32_CASES + EC.BIT16_CASES])
def test_reference_gradients_have_a_scale(name):
    """_nmax and _nrms divide by the reference's max / rms: none may be 0."""
    c = EC.ALL_CASES[name]
    ref, gref, _ = EC.reference(name)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0
    for k in EC.GRADS:
        if k == "edge_biases" and not c.bias:
            continue
        assert np.isfinite(gref[k]).all() and np.abs(gref[k]).max() > 0, k


def test_fused_maxt_data_is_well_conditioned():
    """The T = 16 case's bar (4e-3) is asked of data on which the reference
    itself is well conditioned: its own float32 evaluation within FP32_TOL / 4
    of float64.  The case seed is the first one that meets the rule."""
    c = EC.ALL_CASES["fused_maxt"]
    assert EC.MAXT_FP32_REF_ERR == 1e-3 / 4
    assert EC.reference_fp32_error("fused_maxt") <= EC.MAXT_FP32_REF_ERR
    assert EC.reference_fp32_error("fused_maxt", seed=c.seed) == EC.reference_fp32_error("fused_maxt")
    for s in range(c.seed):
        assert EC.reference_fp32_error("fused_maxt", seed=s) > EC.MAXT_FP32_REF_ERR, s


def test_inputs_are_what_the_paths_need():
    for c in EC.ALL_CASES.values():
        x = EC.inputs(c.name)
        A = x["A"]
        assert A.shape == (c.b, c.C, c.v, c.v) and set(np.unique(A)) <= {0.0, 1.0}
        if c.kind in ("tree", "edges"):
            n = sum(len(g) for g in x["graphs"])
            assert 0 < n <= c.b * c.v            # pair mode's precondition (edges <= b * v)
            assert c.C % 2 == 0
        if c.kind == "edges":
            assert c.h % 4 == 0
        if not c.bias:
            assert not x["w"]["edge_biases"].any()
    for c in EC.TIER_CASES + EC.EMPTY_CASES + EC.BIT16_CASES:
        assert c.h in (128, 256) and c.v <= 128 and not c.generic
    for c in EC.EXTRA_CASES:
        if c.generic:
            assert c.h not in (128, 256) or c.name.startswith("gen_h128_forced")


def test_tier_table_reaches_every_tier():
    spec = [c for c in EC.TIER_CASES + EC.EXTRA_CASES + EC.EMPTY_CASES if not c.generic]
    t = {c.name: EC.tiers(c) for c in spec}

    def reached(key, names=None):
        return {t[n][key] for n in (names or t)}

    tier = [c.name for c in EC.TIER_CASES]
    assert reached("V", tier) == {32, 64, 128}
    assert reached("fused", tier) == {True, False}
    assert reached("rt", tier) == {1, 2}
    assert reached("big", tier) == {True, False}
    assert reached("kc64", tier) == {True, False}
    assert reached("in_place", tier) == {True, False}
    assert reached("dense", tier) == {True, False}
    assert {"k_fwd_fused", "k_gru_fwd2", "k_gru_fwd<256,2>", "k_gru_fwd<128,1>", "k_gru_fwd<128,2>"} \
        <= reached("gru_fwd", tier)
    # both hidden sizes at every padded width
    assert {(c.h, t[c.name]["V"]) for c in EC.TIER_CASES} == {(h, V) for h in (128, 256) for V in (32, 64, 128)}
    # the rows of the issue's table, one by one
    x = t["n32_c1_t1"]
    assert (x["N"], x["dense"], x["rt"], x["KC"], x["kc64"], x["gru_grid"], x["nchunks"]) == (32, False, 1, 32, False, 1, 1)
    assert EC.ALL_CASES["n32_c1_t1"].C == 1 and EC.ALL_CASES["n32_c1_t1"].v == 1
    assert t["dense_t1"]["first_and_last"] and t["dense_t1"]["N"] == 32 and EC.ALL_CASES["dense_t1"].b == 1
    x = t["h256_n64"]
    assert (x["gru_fwd"], x["big"], x["KC"], EC.ALL_CASES["h256_n64"].C % 2) == ("k_gru_fwd<256,2>", False, 64, 1)
    assert (t["v33"]["V"], t["v33"]["N"]) == (64, 192)
    assert (t["v31"]["V"], t["v31"]["dense"]) == (32, False)
    assert (t["v64"]["V"], t["v64"]["dense"]) == (64, True)
    x = t["v65_fused_b1"]
    assert (x["V"], x["fused"], x["dense"], EC.ALL_CASES["v65_fused_b1"].b) == (128, True, False, 1)
    x = t["dense_sd_256"]
    assert (x["dense"], x["fused"], x["in_place"], x["gru_fwd"], x["big"], x["KC"]) == \
        (True, False, False, "k_gru_fwd2", True, 128)
    x = t["dense_sd_128"]
    assert (x["dense"], x["fused"], x["in_place"]) == (True, False, False)
    for n in ("fused_t1_c1", "fused_t1_c1_sd"):
        assert (t[n]["fused"], t[n]["dense"], t[n]["first_and_last"]) == (True, True, True)
        assert EC.ALL_CASES[n].C == 1 and EC.ALL_CASES[n].T == 1
    assert t["fused_t1_c1_sd"]["sbits"] and not t["fused_t1_c1"]["sbits"]
    assert (t["v127_128"]["V"], t["v127_256"]["V"]) == (128, 128)
    assert not t["v127_128"]["dense"] and not t["v127_256"]["dense"]
    assert t["ed_cpt2"]["cpt"] == 2
    assert t["fused_maxt"]["fused"] and EC.ALL_CASES["fused_maxt"].T + 1 > EC.FUSED_MAXT
    # a backward at b = 1 and the empty-channel shapes
    assert any(c.b == 1 for c in EC.TIER_CASES)
    assert not t["empty_n192"]["big"] and t["empty_n192"]["N"] % 128 != 0
    assert t["empty_lists"]["lists"] and not EC.tiers(EC.ALL_CASES["empty_lists"], skip=False)["lists"]
    # state dropout: fused (keep bits) and unfused, padded and dense
    sd = {(x["fused"], x["dense"]) for n, x in t.items() if EC.ALL_CASES[n].sk < 1.0}
    assert sd == {(True, True), (True, False), (False, True), (False, False)}
