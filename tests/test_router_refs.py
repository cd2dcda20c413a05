"""CPU: the checks of the router kernel tests (tests/router_cases.py, run on the GPU by tests/test_router_kernels_gpu.py) can fail.
Every case is exact in fc1 and its tolerance, 8 x the f32 restatements' own error, stays below LOGIT_TOL / 10; every wrong-kernel
stand-in moves the rows meant to catch it by at least 10 x that tolerance; the float64 reference agrees with the reference project's
recorded logits (tests/golden/router.json) on the three dataset shapes."""
import json
import os

import numpy as np
import pytest

from tests import router_cases as R


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_tolerance_condition(name):
    """8 x e32(case) <= LOGIT_TOL / 10 = 2e-5, and the f32 restatements do differ from float64 (the measurement measures something)."""
    c = R.case(name)
    print(f"router case {name}: nq {c.nq} d_max {c.w.d_max} sources {c.w.n_sources} e32 {c.e32:.3g} tolerance {c.tol:.3g}")
    assert 0 < c.e32 and c.tol <= R.TOL_CAP, (name, c.e32)
    assert np.isfinite(c.ref).all() and np.abs(c.ref).max() < 16


_CATCHERS = R.catchers()


def test_every_stand_in_has_rows_that_catch_it():
    assert {n for n, _, _ in _CATCHERS} == set(R.STAND_INS)


@pytest.mark.parametrize("i", range(len(_CATCHERS)), ids=[f"{n}@{c}#{i}" for i, (n, c, _) in enumerate(_CATCHERS)])
def test_stand_in_is_rejected(i):
    """On every query row named for it, the wrong kernel's logits are at least 10 x the case's tolerance from the reference (on at
    least one of the named sources): the GPU comparison at 1 x the tolerance cannot pass such a kernel."""
    stand_in, name, (rows, cols) = _CATCHERS[i]
    c = R.case(name)
    assert len(rows) and len(cols)
    diff = np.abs(R.STAND_INS[stand_in](c.w, c.xq) - c.ref)[np.asarray(rows)][:, np.asarray(cols)]
    worst = diff.max(1)
    assert (worst >= 10 * c.tol).all(), (stand_in, name, float(worst.min()), c.tol)


def test_stand_ins_that_need_their_regime():
    """The benign regime does not tell the LayerNorm variants apart at the old tolerance; the cases built for them do."""
    c = R.case("ragged")           # variance of hundreds, mean near 0
    for s in ("eps outside the square root", "one-pass variance in f32"):
        assert np.abs(R.STAND_INS[s](c.w, c.xq) - c.ref).max() < R.LOGIT_TOL
    small, big = R.case("layernorm:small-variance"), R.case("layernorm:mean-4096")
    assert np.abs(R.STAND_INS["eps outside the square root"](small.w, small.xq) - small.ref)[:16].max() > 1e-3
    assert np.abs(R.STAND_INS["one-pass variance in f32"](big.w, big.xq) - big.ref)[:16].max() > 10 * big.tol


def test_constant_row_gives_relu_of_the_bias():
    """w1q = 0 and a constant c1 row: x - mean is exactly 0, so h1 = relu(ln1_b) for every query and source, in float64 and in f32."""
    c = R.case("layernorm:constant-row")
    w = c.w
    assert not w.w1q.any() and (np.ptp(w.c1, axis=1) == 0).all()
    assert np.array_equal(R._ln64(np.full((1, 256), 3.0), w.ln1_g, w.ln1_b, 1e-5)[0], w.ln1_b.astype(np.float64))
    assert np.ptp(c.ref) == 0 and abs(c.ref[0, 0] - R._head64(w, np.full((1, 1, 256), 3.0))[0, 0]) < 1e-14    # (BLAS block shapes)


@pytest.mark.parametrize("thr", ("0.4924", "0.5"))
def test_mask_cases_straddle_the_boundary(thr):
    c = R.case(f"mask:{thr}")
    p = R.sigmoid64(c.ref)
    on_boundary = np.abs(p - np.float64(c.w.thr)) <= 2 * R.MASK_MARGIN       # the reference alone, with room for the kernels' error
    assert on_boundary.mean() <= 0.005
    keep = R.mask_of(c.w, c.ref)
    assert 0.3 < keep.mean() < 0.7
    wrong = R.mask_ignoring_threshold(c.w, c.ref)
    if thr == "0.4924":
        assert (wrong != keep)[~on_boundary].any(), "logit > 0 ignores prob_threshold: it must differ off the boundary"
    else:
        assert np.array_equal(wrong, keep)
    for b3, want in ((200.0, True), (-200.0, False)):
        assert (R.mask_of(c.w, R.folded_forward64(c.w.replace(b3=b3), c.xq)[0]) == want).all()


@pytest.mark.parametrize("column", R.NAN_COLUMNS)
def test_reference_keeps_a_nan_to_its_rows(column):
    base = R.case("nan-base")
    got = R.folded_forward64(base.w, R.with_nan(base, column))[0]
    hit = np.zeros(got.shape, bool)
    hit[R.NAN_QUERY, R.rows_on_model(base.w, 0)] = True
    assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], base.ref[~hit])
    assert not R.mask_of(base.w, got)[hit].any()
    g0 = R.NAN_QUERY - R.NAN_QUERY % 4
    assert not base.xq[g0:g0 + 4, 0, 100:].any() and not base.xq[R.NAN_QUERY, 0].any()


def test_case_layouts():
    """What the GPU cases rely on: the column rows are one-hot in every column; the tiles case has a tile without a live chunk and a
    tile whose queries differ in their live chunks; the tails start where they are said to, mixed inside groups and the tile."""
    for d in R.COLUMN_WIDTHS:
        x = R.case(f"columns:{d}").xq
        assert x.shape[0] == d + 38 and np.array_equal(x[:d, 0], np.eye(d)) and np.array_equal(x[:d, 1], np.eye(d)[::-1])
        assert not x[d].any() and np.abs(x[d + 1:]).max() == 2
    t = R.case("tiles").xq
    assert not t[64:128, 0].any() and t[64:128, 1].any() and not t[128:, 1].any()
    assert t[128::2, 0, :128].any() and not t[128::2, 0, 128:].any() and t[129::2, 0, 128:].any() and not t[129::2, 0, :128].any()
    tails = R.case("tails")
    x, starts = tails.xq, tails.meta["starts"]
    for q in range(x.shape[0]):
        for m in range(2):
            nz = np.flatnonzero(x[q, m])
            assert (nz[-1] + 1 if nz.size else 0) == starts[q, m]
    assert all(len(set(starts[g:g + 4, 0])) >= 3 for g in range(0, 68, 4)) and set(starts[:64, 0]) == set(R.TAIL_STARTS) | {770}
    m = R.case("max-width")
    assert m.w.d_max == 8191 and m.xq[0, 0, -1] != 0 and m.xq[1, 0, 0] != 0 and (np.count_nonzero(m.xq, axis=2) == 1).all()


@pytest.mark.parametrize("dataset", ["medrag", "feb4rag", "wikipedia"])
def test_reference_agrees_with_the_recorded_reference_logits(dataset):
    """folded_forward64 on synth_router_case weights folded by fold_weights (rounded to f32, as the device gets them) agrees with
    the logits the reference project computed (tests/golden/router.json) within LOGIT_TOL."""
    from ragroute_amd import config as C
    from ragroute_amd.router import Router, fold_weights
    from tests.util import synth_router_case
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "router.json")))[dataset]
    case = synth_router_case(dataset, g["seed"])
    sources, d_max, sd = case["sources"], case["d_max"], case["sd"]
    r = Router(dataset, sources, "ragroute")
    ids = {"medrag": C.MEDRAG_SOURCE_TO_ID, "feb4rag": C.FEB4RAG_SOURCE_TO_ID}.get(dataset)
    onehot = [ids[c] for c in sources] if ids else [int(c) for c in sources]
    mos = [r.model_names.index(C.EMBEDDING_MODELS_PER_DATA_SOURCE[dataset][c][0]) for c in sources]
    mean, scale = case["scaler"] if case["scaler"] is not None else (None, None)
    cents = np.stack([np.pad(case["centroids"][c], (0, d_max - len(case["centroids"][c]))) for c in sources])
    w1q, c1 = fold_weights(sd, cents, onehot, len(ids) if ids else len(sources), d_max, mean, scale)
    w = R.Weights(mos, b3=sd["fc3.bias"][0], thr=C.ROUTER_THRESHOLD[dataset], w1q=w1q, c1=c1, ln1_g=sd["ln1.weight"], ln1_b=sd["ln1.bias"],
                  w2=sd["fc2.weight"].T, b2=sd["fc2.bias"], ln2_g=sd["ln2.weight"], ln2_b=sd["ln2.bias"], w3=sd["fc3.weight"].reshape(-1))
    xq = np.concatenate([r.pack_queries(q).numpy() for q in case["queries"]])
    got = R.folded_forward64(w, xq)[0]
    want = np.asarray(g["logits"], np.float64)
    assert got.shape == want.shape and np.abs(got - want).max() < R.LOGIT_TOL, float(np.abs(got - want).max())
    names = [[c for c, keep in zip(sources, row) if keep] for row in R.mask_of(w, got)]
    boundary = np.log(float(w.thr) / (1 - float(w.thr)))
    for row, sel, want_sel in zip(want, names, g["selected"]):
        for c, wl in zip(sources, row):
            if abs(wl - boundary) > R.LOGIT_TOL:
                assert (c in sel) == (c in want_sel)
