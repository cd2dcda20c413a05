"""GPU: the three router MLP kernels (csrc/router.hip) against the float64 statement of tests/router_cases.py, through the C ABI.

Every case runs through the small form (rr_router_mlp: router_mlp_kernel at any batch size) and, from 32 queries on where the
topology allows, through the matrix-core form (rr_router_mlp_ws with a workspace: router_fc1_kernel + router_head_kernel); which form
ran is asserted from rr_router_workspace_bytes.  Outputs are slices of sentinel-filled buffers (NaN-pattern logits, mask bytes 0xAB,
one spare row before and after, 4 KiB behind the workspace) whose surroundings must stay untouched; each form must be bit-identical
when run twice and within the case's tolerance of folded_forward64.  The tolerance is 8 x e32(case), measured from the reference
alone (router_cases.py) and capped at LOGIT_TOL / 10 = 2e-5 by tests/test_router_refs.py.

Measured on an MI355X (every run prints the figures before it asserts): e32, tolerance = 8 x e32, largest deviation of the small
form and of the matrix-core form over all batch sizes of the case.
    columns:1                          4.55e-07 3.64e-06 2.14e-07 3.53e-07
    columns:4                          7.15e-07 5.72e-06 3.67e-07 3.75e-07
    columns:100                        7.97e-07 6.37e-06 4.12e-07 6.16e-07
    columns:128                        6.86e-07 5.49e-06 3.87e-07 4.79e-07
    columns:130                        9.89e-07 7.91e-06 4.52e-07 5.49e-07
    columns:132                        9.21e-07 7.37e-06 3.99e-07 4.54e-07
    columns:770                        6.93e-07 5.54e-06 4.01e-07 5.53e-07
    tiles                              7.39e-07 5.91e-06 3.45e-07 4.29e-07
    ragged                             1.06e-06 8.50e-06 4.57e-07 5.93e-07
    topology:1x1                       4.02e-07 3.22e-06 3.80e-07    -
    topology:5x1                       9.03e-07 7.23e-06 4.04e-07    -
    topology:8x1                       6.07e-07 4.86e-06 3.64e-07 4.00e-07
    topology:9-on-model-0-of-2         7.07e-07 5.66e-06 3.18e-07 4.53e-07
    topology:33x3-interleaved          6.40e-07 5.12e-06 3.50e-07 5.07e-07
    layernorm:small-variance           4.79e-07 3.83e-06 3.56e-07 4.01e-07
    layernorm:mean-4096                4.69e-07 3.75e-06 3.54e-07 3.18e-07
    layernorm:constant-row             1.89e-07 1.51e-06 9.96e-09 2.48e-07
    tails                              5.75e-07 4.60e-06 3.13e-07 4.37e-07
    nan-base                           4.97e-07 3.98e-06 3.51e-07 5.56e-07
    mask:0.4924                        7.88e-07 6.30e-06 3.20e-07 4.08e-07
    mask:0.5                           6.59e-07 5.27e-06 2.75e-07 4.01e-07
    max-width                          3.91e-07 3.13e-06 2.52e-07 2.69e-07
Two defects were found by these cases and fixed in csrc/router.hip.  columns:770, small form, deviated by 0.279: the k loop of
router_mlp_kernel ended at the column a thread saw LAST, not at the furthest one, once a thread visits several inputs (4 d_max >
1024) - router_cases.thread_last_kend restates it and gives the same 0.279.  The NaN cases returned finite logits: fmaxf(NaN, 0) = 0
made a NaN embedding a row of zeros after the first ReLU; both forms now give such a row a NaN logit.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import router_cases as R

pytestmark = pytest.mark.gpu
RR_OK, RR_ERR_WORKSPACE = 0, -3
WS_GUARD = 4096


class Device:
    """Weights of a case on the device: FoldedRouter on the hand-made arrays, n_models set in the struct where it exceeds
    max(model_of_source) + 1."""

    def __init__(self, w):
        from ragroute_amd._lib import lib
        from ragroute_amd.router import FoldedRouter
        self.w, self.L = w, lib()
        self.fr = FoldedRouter(w.w1q, w.c1, w.state_dict(), [int(m) for m in w.model_of_source], float(w.thr))
        self.fr.struct.n_models = w.n_models
        assert self.fr.struct.d_max == w.d_max and self.fr.struct.n_sources == w.n_sources
        assert np.float32(self.fr.struct.b3) == w.b3 and np.float32(self.fr.struct.prob_threshold) == w.thr

    def ws_bytes(self, nq):
        return self.L.rr_router_workspace_bytes(ctypes.byref(self.fr.struct), nq)

    def run(self, xq, form, ws_short=0, expect=RR_OK):
        """(logits f32 [nq][C], mask u8 [nq][C]) as numpy, after checking the sentinels around them.  xq: device f32 [nq][M][d_max]."""
        nq, C = xq.shape[0], self.w.n_sources
        assert xq.is_contiguous() and xq.shape[1:] == (self.w.n_models, self.w.d_max)
        lbuf = torch.full((nq + 2, C), R.NAN_LOGIT_BITS, dtype=torch.int32, device=xq.device)
        mbuf = torch.full((nq + 2, C), R.MASK_SENTINEL, dtype=torch.uint8, device=xq.device)
        lout, mout = lbuf[1:nq + 1], mbuf[1:nq + 1]
        st = torch.cuda.current_stream().cuda_stream
        need = self.ws_bytes(nq)
        if form == "small":
            rc = self.L.rr_router_mlp(ctypes.byref(self.fr.struct), xq.data_ptr(), nq, lout.data_ptr(), mout.data_ptr(), st)
        else:
            assert need > 0, "this case must take the matrix-core form"
            ws = torch.full((need + WS_GUARD,), R.MASK_SENTINEL, dtype=torch.uint8, device=xq.device)
            rc = self.L.rr_router_mlp_ws(ctypes.byref(self.fr.struct), xq.data_ptr(), nq, lout.data_ptr(), mout.data_ptr(), ws.data_ptr(),
                                         need - ws_short, st)
            torch.cuda.synchronize()
            assert bool((ws[need:] == R.MASK_SENTINEL).all()), "a kernel wrote behind its workspace"
            if expect != RR_OK:
                assert bool((ws == R.MASK_SENTINEL).all()), "a refused call wrote to the workspace"
        torch.cuda.synchronize()
        assert rc == expect, (rc, self.L.rr_last_error())
        lall, mall = lbuf.cpu().numpy(), mbuf.cpu().numpy()
        for part in (lall[:1], lall[nq + 1:]):
            assert (part == R.NAN_LOGIT_BITS).all(), "a kernel wrote logits outside its rows"
        for part in (mall[:1], mall[nq + 1:]):
            assert (part == R.MASK_SENTINEL).all(), "a kernel wrote mask bytes outside its rows"
        if expect != RR_OK:
            assert (lall == R.NAN_LOGIT_BITS).all() and (mall == R.MASK_SENTINEL).all(), "a refused call wrote to its outputs"
            return None, None
        assert not (lall[1:nq + 1] == R.NAN_LOGIT_BITS).any() and np.isin(mall[1:nq + 1], (0, 1)).all(), "every output is written"
        return lall[1:nq + 1].view(np.float32).copy(), mall[1:nq + 1].copy()

    def run_twice(self, xq, form):
        a, b = self.run(xq, form), self.run(xq, form)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]), f"{form} form: two runs differ"
        return a


def forms(dev, nq, mfma_expected=None):
    """The forms a batch of nq queries runs through; which one rr_router_mlp_ws picks is asserted where the case states it."""
    has = dev.ws_bytes(nq) > 0
    if mfma_expected is not None:
        assert has == mfma_expected, (nq, dev.ws_bytes(nq))
    assert not (has and nq < 32), "the matrix-core form is never taken below 32 queries"
    return ("small", "mfma") if has else ("small",)


def check_logits(case, got, rows, form, what=""):
    """got f32 [len(rows)][C] against the case's reference rows, at the case's tolerance; prints the figures before it asserts."""
    ref = case.ref[rows]
    dev = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"ROUTER-DEV {case.name}{what} form={form} nq={got.shape[0]} e32={case.e32:.3g} tol={case.tol:.3g} max_dev={dev:.3g}")
    assert dev <= case.tol, (case.name, form, dev, case.tol)


def check_mask(w, logits, mask, max_skipped=0.01):
    """mask == (sigmoid64(gpu logit) > thr) wherever the probability is further than MASK_MARGIN from the threshold."""
    p = R.sigmoid64(logits)
    off = np.abs(p - np.float64(w.thr)) > R.MASK_MARGIN
    assert (~off).mean() <= max_skipped, float((~off).mean())
    assert np.array_equal(mask[off].astype(bool), (p > np.float64(w.thr))[off])


def run_case(case, gpu, nqs=None, mfma_expected=None):
    """Every batch size (a prefix of the case's queries) through every form it can take; returns {(nq, form): (logits, mask)}."""
    dev = Device(case.w)
    xq = torch.from_numpy(case.xq).to(gpu)
    out = {}
    for nq in (nqs or [case.nq]):
        for form in forms(dev, nq, None if mfma_expected is None else mfma_expected and nq >= 32):
            logits, mask = dev.run_twice(xq[:nq], form)
            check_logits(case, logits, slice(0, nq), form)
            check_mask(case.w, logits, mask)
            out[nq, form] = logits, mask
    return out


@pytest.mark.parametrize("d_max", R.COLUMN_WIDTHS)
def test_every_column_reaches_fc1(gpu, d_max):
    """One one-hot row per column (model 1 mirrored), an all-zero row, dense rows: both load paths of router_fc1_kernel (d_max % 4),
    its partial last chunk (d_max % 128), every quarter boundary of the small kernel's k range, tiles with one live chunk."""
    out = run_case(R.case(f"columns:{d_max}"), gpu, mfma_expected=True)
    assert set(out) == {(d_max + 38, "small"), (d_max + 38, "mfma")}


def test_tiles_without_and_with_different_live_chunks(gpu):
    """A 64-query tile whose model-0 embeddings are all zero (no live chunk: fc1 = c1[c]), and a tile whose queries have different
    live chunks (valid[] / vlist / nvalid are per tile, not per query)."""
    run_case(R.case("tiles"), gpu, mfma_expected=True)


def test_ragged_batches(gpu):
    """nq around the group of 4, the 32-row head block and the 64-query tile; 13 sources on 8 models.  One reference of 129 rows."""
    out = run_case(R.case("ragged"), gpu, nqs=R.RAGGED_NQ, mfma_expected=True)
    assert sum(1 for _, form in out if form == "mfma") == sum(1 for nq in R.RAGGED_NQ if nq >= 32)
    full = out[129, "small"][0]
    for (nq, form), (logits, _) in out.items():      # exact fc1: a query's result does not depend on the batch it came in
        if form == "small":
            assert np.array_equal(logits.view(np.uint32), full[:nq].view(np.uint32)), nq


@pytest.mark.parametrize("topology", list(R.TOPOLOGIES))
def test_topologies(gpu, topology):
    """Source-to-model mappings at 5 and 70 queries: one source; the (n_models == 1, fewer than 8 sources) fall-back to the small
    kernel at 70 queries and its first exception; a model without sources; an unsorted mapping with an unused model in the middle
    and 17 sources on one model (the wave slots cycle four times)."""
    mfma = R.TOPOLOGIES[topology][2]
    out = run_case(R.case(f"topology:{topology}"), gpu, nqs=(5, 70), mfma_expected=mfma)
    assert ((70, "mfma") in out) == mfma and (5, "mfma") not in out


@pytest.mark.parametrize("regime", ["small-variance", "mean-4096", "constant-row"])
def test_layernorm_regimes(gpu, regime):
    """Variance near eps (eps outside the square root moves these logits by 4e-3), a mean of 4096 over a variance of 24 (one-pass
    f32 variance fails here), and a constant fc1 row (x - mean = 0 exactly: h1 = relu(ln1_b))."""
    case = R.case(f"layernorm:{regime}")
    out = run_case(case, gpu, mfma_expected=True)
    if regime == "constant-row":
        for logits, _ in out.values():
            assert np.ptp(logits) == 0, "every (query, source) row has the same h1 = relu(ln1_b)"


def test_zero_padded_tails(gpu):
    """Embeddings zero from column p on, mixed inside groups of 4 and inside the 64-query tile.  On this exact-fc1 data the zero
    skipping cannot change a bit: each query's small-form logits equal those of the same query sent alone and sent beside a
    full-width neighbour, and its matrix-core logits do not depend on which queries share its tile."""
    case = R.case("tails")
    out = run_case(case, gpu, mfma_expected=True)
    dev = Device(case.w)
    xq = torch.from_numpy(case.xq).to(gpu)
    batched, bmask = out[case.nq, "small"]
    full = xq[6:7]                                    # a full-width query
    assert case.meta["starts"][6].tolist() == [770, 770]
    for q in range(case.nq):
        alone, amask = dev.run(xq[q:q + 1].contiguous(), "small")
        pair, pmask = dev.run(torch.cat([xq[q:q + 1], full]), "small")
        for got, m in ((alone[0], amask[0]), (pair[0], pmask[0])):
            assert np.array_equal(got.view(np.uint32), batched[q].view(np.uint32)) and np.array_equal(m, bmask[q]), q
    perm = np.random.default_rng(3).permutation(case.nq)
    shuffled, smask = dev.run(xq[torch.from_numpy(perm).to(gpu)].contiguous(), "mfma")
    tiled, tmask = out[case.nq, "mfma"]
    assert np.array_equal(shuffled.view(np.uint32), tiled[perm].view(np.uint32)) and np.array_equal(smask, tmask[perm])


@pytest.mark.parametrize("column", R.NAN_COLUMNS)
def test_nan_stays_with_its_query_and_model(gpu, column):
    """A NaN in one query's model-0 embedding: that query's logits on the model-0 sources are NaN with mask 0; every other output
    - its own model-1 sources, its 3 group neighbours (small form), its 63 tile neighbours (matrix-core form) - is bit-identical
    to the run without the NaN.  In the last column the NaN is the only non-zero input past column 100 of its group."""
    base = R.case("nan-base")
    clean = run_case(base, gpu, mfma_expected=True)
    dev = Device(base.w)
    xq = torch.from_numpy(R.with_nan(base, column)).to(gpu)
    hit = np.zeros((base.nq, base.w.n_sources), bool)
    hit[R.NAN_QUERY, R.rows_on_model(base.w, 0)] = True
    for form in ("small", "mfma"):
        logits, mask = dev.run_twice(xq, form)
        want_l, want_m = clean[base.nq, form]
        assert np.isnan(logits[hit]).all() and not mask[hit].any(), form
        assert np.array_equal(logits[~hit].view(np.uint32), want_l[~hit].view(np.uint32)) and np.array_equal(mask[~hit], want_m[~hit]), form


@pytest.mark.parametrize("thr", ["0.4924", "0.5"])
def test_mask_follows_logit_and_threshold(gpu, thr):
    """Logits on both sides of the boundary: mask == (sigmoid64(gpu logit) > thr) off a 1e-6 margin (checked by run_case for every
    case; here at most 1 % of the entries may be that close).  b3 = +200 selects everything, b3 = -200 nothing (expf overflows to
    +inf, p = 0).  There the logits are within the case's tolerance plus one rounding of the final sum, whose magnitude is in [128, 256)."""
    case = R.case(f"mask:{thr}")
    out = run_case(case, gpu, mfma_expected=True)
    for logits, mask in out.values():
        assert 0.3 < mask.mean() < 0.7
    xq = torch.from_numpy(case.xq).to(gpu)
    for b3, want in ((200.0, 1), (-200.0, 0)):
        w = case.w.replace(b3=b3)
        dev = Device(w)
        ref = R.folded_forward64(w, case.xq)[0]
        for form in ("small", "mfma"):
            logits, mask = dev.run_twice(xq, form)
            assert (mask == want).all(), (b3, form)
            assert np.abs(logits.astype(np.float64) - ref).max() <= case.tol + 2.0 ** -17      # half an ulp of [128, 256)


def test_arguments_and_the_widest_header(gpu):
    """A workspace one byte short is RR_ERR_WORKSPACE and writes nothing; nq = 0 needs no buffers; the largest accepted d_max
    (8191: 163 824 + 16 bytes of LDS, exactly the 160 KiB of a workgroup) is served by the small form at 1 and 5 queries and by the
    matrix-core form (8 sources, 1 model, 64 chunks, the scalar load path) at 33, on rows one-hot at the last and the first column."""
    small = R.case("ragged")
    dev = Device(small.w)
    xq = torch.from_numpy(small.xq[:40]).to(gpu)
    dev.run(xq, "mfma", ws_short=1, expect=RR_ERR_WORKSPACE)
    assert b"workspace" in dev.L.rr_last_error()
    assert dev.L.rr_router_mlp(ctypes.byref(dev.fr.struct), None, 0, None, None, None) == RR_OK
    assert dev.L.rr_router_mlp_ws(ctypes.byref(dev.fr.struct), None, 0, None, None, None, 0, None) == RR_OK
    assert dev.ws_bytes(0) == 0 and dev.ws_bytes(31) == 0 and dev.ws_bytes(32) > 0
    out = run_case(R.case("max-width"), gpu, nqs=(1, 5, 33), mfma_expected=True)
    assert set(out) == {(1, "small"), (5, "small"), (33, "small"), (33, "mfma")}
