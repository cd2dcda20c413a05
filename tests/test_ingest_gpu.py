"""GPU: the ingest kernels against plain references, through the C ABI - rr_rows_to_half (bit for bit against round-to-nearest-even on
every fp16 / bf16 value, tie and threshold; every path of the kernel), rr_l2_normalize_f32 and the normalising ingest (a derived
relative bound; faiss' edge rows bit for bit), rr_half_sqnorms and rr_centroid (bit for bit on exact data).  Every output is a slice
of a sentinel-filled buffer whose surroundings must stay untouched.  Inputs, references, bounds: tests/ingest_cases.py; that the
checks can fail: tests/test_ingest_refs.py."""
import numpy as np
import pytest
import torch

from tests import ingest_cases as C

pytestmark = pytest.mark.gpu

# (d, ld_in, d_out): d % 4 != 0 takes the scalar path, ld_in % 4 != 0 (or d_out % 4 != 0) alternates the path row by row
SHAPES = [(768, 768, 768), (100, 100, 128), (301, 301, 384), (300, 303, 384), (8, 8, 128), (1, 1, 128), (8192, 8192, 8192), (64, 67, 70)]
MAX_OUT_BYTES = 32 << 20


def _rows_to_half(dev, flat, n, d, ld, d_out, dtype, normalize, offset=0):
    """flat: the f32 input, exactly (n - 1) ld + d floats -> the [n, d_out] output as uint16 patterns.  offset: floats the device
    buffer's base is shifted by (1: no row is 16-byte aligned)."""
    from ragroute_amd._lib import check, lib
    assert flat.size == (n - 1) * ld + d
    buf = torch.empty(offset + flat.size, dtype=torch.float32, device=dev)
    buf[offset:].copy_(torch.from_numpy(flat))
    out = C.Guarded((n, d_out), C.torch_dtype(dtype), dev)
    check(lib().rr_rows_to_half(buf[offset:].data_ptr(), n, d, ld, out.out.data_ptr(), C.RR_DTYPE[dtype], d_out, normalize, None), "rr_rows_to_half")
    out.check()
    return out.bits()


def _convert_all(dev, vals, d, ld, d_out, dtype, n=None, offset=0):
    """The value stream through rr_rows_to_half(normalize = 0) at one shape, in calls of at most MAX_OUT_BYTES of output."""
    flat, x = C.lay_rows(vals, d, ld, n)
    step = max(1, MAX_OUT_BYTES // (2 * d_out))
    for a in range(0, x.shape[0], step):
        b = min(x.shape[0], a + step)
        got = _rows_to_half(dev, flat[a * ld: (b - 1) * ld + d], b - a, d, ld, d_out, dtype, 0, offset)
        assert not got[:, d:].any(), "columns d .. d_out must be +0"
        C.check_half_bits(got[:, :d], x[a:b], dtype)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_rows_to_half_rounds_to_nearest_even(gpu, shape, dtype):
    _convert_all(gpu, C.stream(dtype), *shape, dtype)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_rows_to_half_row_counts_and_unaligned_base(gpu, dtype):
    vals = C.stream(dtype)
    for n in (1, 5, C.BIG_N):                                   # the last: a second grid-stride pass
        _convert_all(gpu, vals, 8, 8, 128, dtype, n=n)
    _convert_all(gpu, vals[: 37 * 768], 768, 768, 768, dtype, offset=1)
    _convert_all(gpu, vals[: 999 * 8], 8, 8, 128, dtype, offset=1)
    _convert_all(gpu, vals[: 41 * 300], 300, 304, 384, dtype, offset=1)


def _normalise_cases():
    for d in (1, 77, 100, 768, 4096):
        yield d, 37
    yield 8, C.BIG_N


@pytest.mark.parametrize("d,n", list(_normalise_cases()))
def test_normalisation_within_the_derived_bound(gpu, d, n):
    from ragroute_amd._lib import check, lib
    rng = np.random.default_rng(100 * d + 1)
    for x in (C.normal_rows(rng, n, d), C.dominant_rows(rng, n, d)):
        g = C.Guarded((n, d), torch.float32, gpu)
        g.out.copy_(torch.from_numpy(x))
        check(lib().rr_l2_normalize_f32(g.out.data_ptr(), n, d, None), "rr_l2_normalize_f32")
        g.check()
        C.check_normalized_f32(g.out.cpu().numpy(), x)
        dim = -(-d // 128) * 128
        for dtype in C.DTYPES:
            got = _rows_to_half(gpu, x.reshape(-1), n, d, d, dim, dtype, 1)
            assert not got[:, d:].any()
            C.check_normalized_half(got[:, :d], x, dtype)


@pytest.mark.parametrize("d", (8, 77, 768))
def test_normalisation_edge_rows_match_faiss_arithmetic(gpu, d):
    from ragroute_amd._lib import check, lib
    x, want = C.edge_rows_expected(d)
    # between ordinary rows, which the bound test covers: here they only have to stay ordinary
    body = C.normal_rows(np.random.default_rng(d), 9, d)
    at = [0, 3, 4, 8]
    body[at] = x
    g = C.Guarded((9, d), torch.float32, gpu)
    g.out.copy_(torch.from_numpy(body))
    check(lib().rr_l2_normalize_f32(g.out.data_ptr(), 9, d, None), "rr_l2_normalize_f32")
    g.check()
    got = g.out.cpu().numpy()
    C.check_bits_equal(got[at], want, "edge rows")
    others = [r for r in range(9) if r not in at]
    C.check_normalized_f32(got[others], body[others])
    dim = -(-d // 128) * 128
    for dtype in C.DTYPES:
        got = _rows_to_half(gpu, body.reshape(-1), 9, d, d, dim, dtype, 1)
        C.check_half_bits(got[at][:, :d], want, dtype)
        C.check_normalized_half(got[others][:, :d], body[others], dtype)


def _half_sqnorms(dev, rows, dtype):
    from ragroute_amd._lib import check, lib
    xb = C.to_half_device(rows, dtype, dev)
    out = C.Guarded((rows.shape[0],), torch.float32, dev, guard=64)
    check(lib().rr_half_sqnorms(xb.data_ptr(), C.RR_DTYPE[dtype], rows.shape[0], rows.shape[1], out.out.data_ptr(), None), "rr_half_sqnorms")
    out.check()
    return out.out.cpu().numpy()


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_half_sqnorms_bit_for_bit(gpu, dtype):
    for name, rows, _ in C.sqnorm_cases(dtype):
        C.check_half_sqnorms(_half_sqnorms(gpu, rows, dtype), rows)
    if dtype == "fp16":
        rows = C.subnormal_rows()
        C.check_half_sqnorms(_half_sqnorms(gpu, rows, dtype), rows)
    else:                                            # |x|^2 / 2 = 2^129 is beyond f32: the norm is +inf, and only that row's
        rows = C.pad_rows(np.ones((5, 100), np.float32), 128)
        rows[3, 17] = 2.0 ** 65
        got = _half_sqnorms(gpu, rows, dtype)
        assert got[3] == np.inf and (got[[0, 1, 2, 4]] == 50).all()
        C.check_half_sqnorms(got, rows)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("n,d,dim", C.CENTROID_CASES)
def test_centroid_bit_for_bit(gpu, n, d, dim, dtype):
    from ragroute_amd._lib import check, lib
    rows = C.centroid_rows(n, d, dim, dtype)
    xb = C.to_half_device(rows, dtype, gpu)
    out = C.Guarded((dim,), torch.float32, gpu, guard=64)
    check(lib().rr_centroid(xb.data_ptr(), C.RR_DTYPE[dtype], n, dim, d, out.out.data_ptr(), None), "rr_centroid")
    out.check()
    C.check_centroid_exact(out.out.cpu().numpy(), rows, d)


def test_centroid_of_inexact_rows(gpu):
    from ragroute_amd._lib import check, lib
    from tests.util import half_round
    n, d, dim = 1000, 700, 768
    rows = C.pad_rows(half_round(np.random.default_rng(4).standard_normal((n, d)).astype(np.float32)), dim)
    xb = C.to_half_device(rows, "fp16", gpu)
    out = C.Guarded((dim,), torch.float32, gpu, guard=64)
    check(lib().rr_centroid(xb.data_ptr(), 0, n, dim, d, out.out.data_ptr(), None), "rr_centroid")
    out.check()
    C.check_centroid_close(out.out.cpu().numpy(), rows, d)
