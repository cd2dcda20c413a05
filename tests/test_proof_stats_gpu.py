"""GPU: what the int8-screen and f32-faithful proofs multiply into their bounds - rr_screen_build's int8 copy and its d_stats words
(max|x|, max|x - s x8|^2, max|x|^2) and rr_faithful_build's Dmax, Xmax, X~max - against f64 references, on corpora where ONE planted
row and column decides each maximum: the first and last row, the rows around a workgroup's four, the rows around the grid-stride
wrap at 32 768, the first and last column, the columns around a lane's 8, a wave's 64 and its 512.  Random data, where every row is
close to the maximum, cannot see a kernel that skips one of them; a proof built on its maxima would certify wrong results.
Corpora, references and bounds: tests/ingest_cases.py; that the checks can fail: tests/test_ingest_refs.py."""
import numpy as np
import pytest
import torch

from tests import ingest_cases as C

pytestmark = pytest.mark.gpu


def _screen_build(dev, rows, dtype):
    """rr_screen_build of stored rows (f32 values of the storage type) -> (x8 int8 [n, dim8], stats f32[8])."""
    from ragroute_amd._lib import check, lib
    n, dim = rows.shape
    dim8 = lib().rr_screen_dim(dim)
    assert dim8 == C.screen_dim8(dim)
    xb = C.to_half_device(rows, dtype, dev)
    x8 = C.Guarded((n, dim8), torch.int8, dev)
    stats = C.Guarded((8,), torch.float32, dev, guard=8)
    check(lib().rr_screen_build(xb.data_ptr(), C.RR_DTYPE[dtype], n, dim, x8.out.data_ptr(), stats.out.data_ptr(), None), "rr_screen_build")
    x8.check()
    stats.check()
    return x8.out.cpu().numpy(), stats.out.cpu().numpy()


SCREEN_SHAPES = [(9, dim) for dim in C.SCREEN_DIMS] + [(C.BIG_N, 128)]


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n,dim", SCREEN_SHAPES)
def test_screen_build_with_planted_outliers(gpu, n, dim, dtype):
    rows_at = C.outlier_rows(n)
    for i, (row, col) in enumerate(C.positions(n, dim)):
        row_e = rows_at[(i + 1) % len(rows_at)]          # the worst-quantising row sits at another of the outlier rows
        x = C.screen_corpus(n, dim, row, col, row_e, nan_before=bool(i % 2))
        assert np.array_equal(C.half_bits_to_f64(C.ref_half_bits(x, dtype), dtype)[~np.isnan(x)], x[~np.isnan(x)])
        x8, stats = _screen_build(gpu, x, dtype)
        assert stats[0] == C.AMAX
        C.check_screen(x, x8, stats)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_screen_build_sees_the_last_chunk_of_a_second_pass(gpu, dtype):
    """max|x| is taken by 4096 x 256 threads striding over 8-element chunks: 32 773 rows of 256 are more chunks than threads, and the
    maximum sits in the very last one."""
    n, dim = C.BIG_N, 256
    assert n * dim // 8 > 4096 * 256
    x = C.screen_corpus(n, dim, n - 1, dim - 1, 0)
    x8, stats = _screen_build(gpu, x, dtype)
    assert stats[0] == C.AMAX
    C.check_screen(x, x8, stats)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_screened_search_never_certifies_a_corpus_with_an_infinity(gpu, dtype):
    """An f32 value beyond the storage type's range is stored as inf.  The int8 scale is then infinite and nothing the screen computes
    is a bound: no served query may be certified, and search() must return what the oracle ranks on the finite rows."""
    from oracle import oracle as O
    from ragroute_amd.flat_index import FlatIndex
    from tests.util import int_data
    rng = np.random.default_rng(8)
    n, d, nq, k, bad = 3000, 100, 9, 10, 1234
    xb, xq = int_data(rng, n, d), int_data(rng, nq, d)
    xb[bad, 40] = 70000.0 if dtype == "fp16" else 3.4e38
    xq[:, 40] = np.where(xq[:, 40] == 0, 1, xq[:, 40])                  # (0 * inf = NaN would hide the row; +-inf must not rank it wrongly)
    idx = FlatIndex(d, dtype=dtype, device=gpu)
    idx.add(xb)
    assert torch.isinf(idx.xb[bad, 40]) and int(torch.isinf(idx.xb).sum()) == 1
    idx.build_screen()
    mask = torch.ones(nq, dtype=torch.uint8, device=gpu)
    mask[4] = 0
    D, I, exact = idx.search_screened(idx.prepare_queries(xq), k, route_mask=mask)
    exact = exact.cpu().numpy()
    assert not exact[mask.cpu().numpy() != 0].any(), "a query was certified against an infinite scale"
    D, I = idx.search(xq, k + 1)
    finite = np.delete(np.arange(n), bad)
    Dr, Ir = O.flat_search_ip(xb[finite], xq, k)
    for q in range(nq):
        keep = I[q] != bad
        assert np.array_equal(I[q][keep][:k], finite[Ir[q]]) and np.array_equal(D[q][keep][:k], Dr[q]), q


def _faithful_build(dev, xf, xh, dtype, dim, ld):
    from ragroute_amd._lib import check, lib
    n, d = xf.shape
    f32 = torch.full((n, ld), -7777.0, dtype=torch.float32, device=dev)
    f32[:, :d] = torch.from_numpy(xf).to(dev)
    xb = C.to_half_device(C.pad_rows(xh, dim), dtype, dev)
    stats = C.Guarded((4,), torch.float32, dev, guard=8)
    check(lib().rr_faithful_build(f32.data_ptr(), ld, xb.data_ptr(), C.RR_DTYPE[dtype], n, d, dim, stats.out.data_ptr(), None), "rr_faithful_build")
    stats.check()
    return stats.out.cpu().numpy()


FAITHFUL_SHAPES = [(9, d) for d in C.FAITHFUL_DIMS] + [(C.BIG_N, 100)]


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n,d", FAITHFUL_SHAPES)
def test_faithful_build_with_planted_outliers(gpu, n, d, dtype):
    from ragroute_amd._lib import lib
    dim = lib().rr_padded_dim(d)
    for i, (row, col) in enumerate(C.positions(n, d, C.FAITHFUL_COLS)):
        xf, xh = C.faithful_corpus(n, d, row, col, dtype, nan_before=bool(i % 2))
        stats = _faithful_build(gpu, xf, xh, dtype, dim, d + 3)          # ld_f32 > d, and no multiple of 4
        C.check_faithful_stats(stats, xf, xh)


def test_faithful_build_row_that_overflows_fp16(gpu):
    n, d = 9, 100
    for row in (0, 8):
        xf, xh = C.faithful_corpus(n, d, 4, 63, "fp16", overflow_row=row)
        assert np.isinf(xh).sum() == 1
        stats = _faithful_build(gpu, xf, xh, "fp16", 128, d + 3)
        assert stats[0] == np.inf and stats[2] == np.inf and np.isfinite(stats[1])
        C.check_faithful_stats(stats, xf, xh)
