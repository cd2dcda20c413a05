"""GPU: ids and scores equal the f64 oracle BIT FOR BIT on data that use every stored mantissa bit and the exponent range.

tests/util.py int_data has values {-2 ... 2}: three bits of an operand reach the matrix cores, and a scan kernel that drops low
mantissa bits, unpacks a fragment through the wrong type or mis-places bytes passes every int_data test.  The exact families
(tests/util.py exact_case; proven exact, order independent and sensitive on the CPU by tests/test_wide_values_data.py) close that:
rows-wide, queries-wide, balanced and power-of-two-scaled integer data for the inner product, the l2 family for the squared-L2
metric, fp16 subnormals, and bf16 rows whose scores overflow f32.

Every half-precision scan kernel, in both storage types, on the dense path and through bootstrap + two chunk launches
(tests/wide_cases.py); the segmented searches of both metrics; the screened search; the f32-faithful bound on subnormal halves is in
tests/test_exact_f32_gpu.py.  Guard-page layouts run in child processes: an over-read is a GPU fault there and must cost one test."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import wide_cases as W
from tests.util import exact_case

pytestmark = pytest.mark.gpu


def _in_child(code, timeout=1500):
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    t0 = time.time()
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout)
    print(res.stdout[-3000:], f"\n[{time.time() - t0:.1f} s in the child]")
    assert res.returncode == 0 and res.stdout.rstrip().endswith("ok"), (res.returncode, res.stdout[-3000:], res.stderr[-2000:])


def test_the_cases_reach_every_half_precision_scan_kernel(gpu):
    """All five kernels, each in both storage types with every family it serves, in chunk launches and - the three kernels that
    have one (tests/wide_cases.py DENSE_FORMS) - in its dense form; and no sixth name: a new scan kernel fails here until the grid
    reaches it."""
    from ragroute_amd import _lib
    W.assert_kernel_coverage(_lib.lib())


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("mode", ["dense", "chunked"])
def test_flat_search_equals_the_oracle_on_wide_values(gpu, mode, dtype):
    """FlatIndex.add / search (dense) and adopt / search_prepared on the guard-page layout (chunked): every (d, nq) of the grid x
    rows / queries / balanced / scaled (ip) and l2 (metric "l2"; 209 ... 256 queries on wide rows: the row-split kernel's L2 form)."""
    _in_child("import torch\nfrom tests.wide_cases import flat_cases, run_flat_case\nfailed = []\n"
              f"for c in flat_cases():\n    if c['mode'] != {mode!r} or c['dtype'] != {dtype!r}: continue\n"
              "    print('case', c, flush=True)\n    bad = run_flat_case(c, torch.device('cuda:0'))\n    if bad: failed.append((c, bad))\n"
              "print('failed', failed)\nassert not failed\nprint('ok')")


@pytest.mark.parametrize("d,rows,nqs,k", W.SEGMENT_CASES)
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_segmented_search_equals_the_oracle_chain_on_wide_values(gpu, metric, d, rows, nqs, k):
    """SegmentedIndex.search with route masks, gaps poisoned (matrix, and the norms for L2) as tests/test_segments*_gpu.py do, against
    their oracle chains."""
    from tests import test_segments_gpu as TS, test_segments_l2_gpu as TL
    for fam, dtype in W.SEGMENT_DATA[metric]:
        rng = np.random.default_rng(sum(rows) + d + len(fam))
        whole, xq_all = exact_case(rng, sum(rows), max(nqs), d, fam, dtype)
        parts = np.split(whole, np.cumsum(rows)[:-1])
        seg = TS.build(parts, d, gpu, dtype=dtype) if metric == "ip" else TL.build(parts, d, gpu, dtype=dtype)
        for nq in nqs:
            xq = xq_all[:nq]
            mask = rng.integers(0, 2, size=(nq, len(rows))).astype(bool)
            mask[0] = False                    # a query routed nowhere: all padding
            if nq > 1:
                mask[1] = True
            for m in (mask, None):
                D, I = seg.search(xq, k, route_mask=m)
                Dr, Ir = (TS.oracle_chain if metric == "ip" else TL.oracle_chain_l2)(parts, xq, k, m)
                assert np.array_equal(I, Ir), (fam, dtype, nq, np.argwhere(I != Ir)[:5])
                assert np.array_equal(D, Dr), (fam, dtype, nq, np.argwhere(D != Dr)[:5])


@pytest.mark.parametrize("d,n,nq,k", W.SCREEN_CASES)
def test_screened_search_on_wide_values(gpu, d, n, nq, k):
    """build_screen / search_screened: wherever the proof holds (exact = 1) rows and scores are the oracle's - the re-scoring reads
    the half rows through its own loads; the public search, which falls back, equals the oracle for every query.  How often the
    proof holds on this data is printed, not asserted."""
    from oracle import oracle as O
    from ragroute_amd.flat_index import FlatIndex
    for i, fam in enumerate(W.IP_FAMILIES):
        for dtype in W.DTYPES:
            rng = np.random.default_rng(n + nq + i)
            xb, xq = exact_case(rng, n, nq, d, fam, dtype)
            idx = FlatIndex(d, dtype=dtype, device=gpu)
            idx.add(xb)
            idx.build_screen()
            Dr, Ir = O.flat_search_ip(xb, xq, k)
            D, I, exact = (t.cpu().numpy() for t in idx.search_screened(idx.prepare_queries(xq), k))
            ok = exact.astype(bool)
            print(f"screen d={d} {fam} {dtype}: {int(ok.sum())} of {nq} queries proven")
            assert np.array_equal(I[ok], Ir[ok]) and np.array_equal(D[ok], Dr[ok]), (fam, dtype)
            D, I = idx.search(xq, k)
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr), (fam, dtype)


@pytest.mark.parametrize("d,nqs", W.SUBNORMAL_CASES)
def test_fp16_subnormal_rows_score_exactly(gpu, d, nqs):
    """Rows m 2^-24, |m| <= 1023: every stored value an fp16 subnormal, ranked against rows that reach the lowest normal binade.
    The matrix cores must not flush subnormal INPUTS: include/ragroute_hip.h promises scores exact for the stored halves."""
    assert not W.run_subnormal_case(d, nqs, gpu)


# ---- scores that overflow f32 ----------------------------------------------------------------------------------------------------
def _overflow_corpus(rng, n, d, counts):
    """bf16 rows of four kinds, queries all positive (integers 1 ... 3 times 16):
    P  every value in {1, 2, 3} * 2^120: each product is finite, every partial sum grows, the score is +inf in any order;
    M  the negatives of such rows: -inf;
    N  a small-integer row that also stores +inf and -inf (their products are +inf and -inf whatever the arithmetic: NaN), or a NaN;
    F  small integers {-2 ... 2}: finite, exact."""
    kind = np.full(n, "F")
    special = rng.permutation(n)
    o = 0
    for name in "PMN":
        kind[special[o: o + counts[name]]] = name
        o += counts[name]
    xb = rng.integers(-2, 3, size=(n, d)).astype(np.float32)
    big = rng.integers(1, 4, size=(n, d)).astype(np.float32) * np.float32(2.0 ** 120)
    xb[kind == "P"] = big[kind == "P"]
    xb[kind == "M"] = -big[kind == "M"]
    for j, r in enumerate(np.flatnonzero(kind == "N")):
        if j % 2:
            xb[r, rng.integers(0, d)] = np.nan
        else:
            a, b = rng.choice(d, size=2, replace=False)
            xb[r, a], xb[r, b] = np.inf, -np.inf
    return xb, kind


@pytest.mark.parametrize("d,n,nq,k,counts", [
    (768, 300, 8, 200, {"P": 30, "M": 100, "N": 30}),           # dense; k beyond the +inf and finite rows: the -inf rows' turn
    (768, 9_000, 256, 100, {"P": 20, "M": 8_830, "N": 100}),    # chunked; 50 finite rows
    (768, 20_000, 40, 100, {"P": 150, "M": 1_000, "N": 200}),   # more +inf rows than k
    (2048, 20_000, 256, 100, {"P": 40, "M": 1_000, "N": 200}),  # the row-split kernel: two waves' partial sums meet
    (2048, 3_000, 200, 100, {"P": 40, "M": 2_900, "N": 20}),    # wide rows, dense; 40 finite rows
])
def test_scores_that_overflow_f32(gpu, d, n, nq, k, counts):
    """What include/ragroute_hip.h (rr_flat_search) states for scores outside f32's range: ids in range, none twice, a NaN-scoring
    row never returned, +inf rows first by ascending id, then the finite rows in the oracle's order.  A real row scoring -inf: on the
    dense path (a corpus of up to 8192 rows: dense_select_kernel ranks every valid key, and -inf has one) it is returned after the
    finite rows, by ascending id, as (-inf, id); a chunk launch passes a row only if its score is strictly above the query's
    threshold, which starts at -inf, so a larger corpus never returns such a row and the tail is padding (-inf, -1)."""
    from oracle import oracle as O
    from ragroute_amd.flat_index import FlatIndex
    rng = np.random.default_rng(n + d)
    xb, kind = _overflow_corpus(rng, n, d, counts)
    xq = rng.integers(1, 4, size=(nq, d)).astype(np.float32) * 16
    idx = FlatIndex(d, dtype="bf16", device=gpu)
    idx.add(xb)
    D, I = idx.search(xq, k)
    P, M, F = (np.flatnonzero(kind == c) for c in "PMF")
    Df, If = O.flat_search_ip(xb[F], xq, min(k, len(F)))
    n_p, n_f = min(k, len(P)), min(max(0, k - len(P)), len(F))
    n_m = min(k - n_p - n_f, len(M)) if n <= 8192 else 0            # -inf rows returned: the dense path only
    for q in range(nq):
        got = I[q][I[q] >= 0]
        assert np.all(got < n) and len(set(got.tolist())) == len(got)
        assert not np.any(kind[got] == "N")
        assert np.array_equal(I[q, :n_p], P[:n_p]) and np.all(np.isposinf(D[q, :n_p]))
        assert np.array_equal(I[q, n_p: n_p + n_f], F[If[q, :n_f]]) and np.array_equal(D[q, n_p: n_p + n_f], Df[q, :n_f])
        assert np.all(np.isneginf(D[q, n_p + n_f:]))
        tail = I[q, n_p + n_f:]
        assert np.array_equal(tail[:n_m], M[:n_m]) and np.all(tail[n_m:] == -1), (q, n_m, tail[:8])
