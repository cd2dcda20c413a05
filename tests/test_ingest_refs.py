"""CPU: the inputs and checks of the ingest / proof-build kernel tests (tests/ingest_cases.py) can tell a right kernel from a subtly
wrong one.  Every check_* helper the GPU tests use is run here on a numpy stand-in of the right kernel, which it accepts, and of a
wrong one (a truncating or ties-away convert, maxima that skip the last row or the columns past a multiple of 64, a norm that drops
the last 8 columns), which it rejects."""
import numpy as np
import pytest

from tests import ingest_cases as C


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_conversion_stream_tells_rounding_rules_apart(dtype):
    x = C.stream(dtype)
    assert x.dtype == np.float32 and 250_000 < x.size < 400_000
    even, odd = C.tie_parities(x, dtype)
    assert even > 1000 and odd > 1000, "ties with an even and with an odd upper neighbour"
    assert np.isnan(x).any() and np.isinf(x).any() and (x.view(np.uint32) == 0x80000000).any()
    sub = (np.abs(x) > 0) & (np.abs(x) < np.finfo(np.float32).tiny)
    assert sub.any(), "f32 subnormals"
    C.check_half_bits(C.ref_half_bits(x, dtype), x, dtype)
    ref = C.ref_half_bits(x, dtype)
    for wrong in (C.convert_truncate, C.convert_half_up):
        got = wrong(x, dtype)
        off = (got != ref) & ~np.isnan(x)
        assert off.any() and (np.abs(got[off].astype(np.int32) - ref[off].astype(np.int32)) == 1).all(), "a wrong rule is one step off"
        with pytest.raises(AssertionError, match="differ from nearest-even"):
            C.check_half_bits(got, x, dtype)
    # each wrong rule fails on the kind of tie it gets wrong, and only truncation on the inexact values
    a = np.abs(C._f64(x))
    a = np.where(np.isfinite(a) & (a < (65520 if dtype == "fp16" else 2.0 ** 127)), a, 0.0)
    q = C._quantum(a, dtype)
    k = np.floor(a / q)
    tie = (a - k * q) * 2 == q
    assert ((C.convert_truncate(x, dtype) != ref) & tie & (k % 2 == 1)).any()
    assert ((C.convert_half_up(x, dtype) != ref) & tie & (k % 2 == 0)).any()


def test_fp16_stream_holds_the_named_values():
    x = C.fp16_stream()
    for v in (65504.0, 65520.0, np.nextafter(np.float32(65520), np.float32(0)), np.nextafter(np.float32(65520), np.float32(np.inf)),
              2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(0)), np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
              np.finfo(np.float32).max, np.inf, 2.0 ** -24, 2.0 ** -14):
        assert (x == np.float32(v)).any() and (x == -np.float32(v)).any(), v
    bits = C.ref_half_bits(np.array([65519.996, 65520, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1))], np.float32), "fp16")
    assert bits.tolist() == [0x7BFF, 0x7C00, 0x0000, 0x0001]


def test_lay_rows_is_exactly_sized():
    v = np.arange(1, 30, dtype=np.float32)
    flat, x = C.lay_rows(v, 3, 5)
    assert x.shape == (10, 3) and flat.size == 9 * 5 + 3
    assert np.array_equal(flat[5:8], x[1]) and (flat[3:5] == -7777).all() and x[9, 2] == 1


@pytest.mark.parametrize("d", (1, 77, 768))
def test_normalisation_checks(d):
    rng = np.random.default_rng(d)
    for kind, x in (("normal", C.normal_rows(rng, 9, d)), ("dominant", C.dominant_rows(rng, 9, d))):
        ref = C.normalize_ref(x)
        C.check_normalized_f32(ref.astype(np.float32), x)
        for dtype in C.DTYPES:
            C.check_normalized_half(C.ref_half_bits(ref.astype(np.float32), dtype), x, dtype)
        if d >= 77 and kind == "normal":   # a norm that drops the last 8 columns (of 9 rows, at least one feels it)
            x64 = x.astype(np.float64)
            wrong = (x64 / np.sqrt((x64[:, :-8] ** 2).sum(1, keepdims=True))).astype(np.float32)
            with pytest.raises(AssertionError):
                C.check_normalized_f32(wrong, x)
            with pytest.raises(AssertionError):
                C.check_normalized_half(C.ref_half_bits(wrong, "fp16"), x, "fp16")
    # an error of three ulps in a small element of a dominant row: invisible to an absolute 1e-6, rejected here
    if d >= 77:
        x = C.dominant_rows(rng, 4, d)
        got = C.normalize_ref(x).astype(np.float32)
        j = int(np.argmin(np.abs(got[0])))
        assert abs(got[0, j]) < 2e-3
        got[0, j] = np.float32(got[0, j] * (1 + (d / 2 + 12) * C.U))
        assert np.allclose(got, C.normalize_ref(x), atol=1e-6, rtol=0)
        with pytest.raises(AssertionError):
            C.check_normalized_f32(got, x)


def test_edge_rows_under_the_oracle():
    for d in (8, 77):
        x, want = C.edge_rows_expected(d)
        assert np.isnan(want[2]).sum() == 1 and (want[0] == 0).all() and (np.abs(want[1]) == 2.0 ** -80).all()


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_sqnorm_cases_are_exact_and_sensitive(dtype):
    for name, rows, exp in C.sqnorm_cases(dtype):
        if rows.shape[0] > 100:
            rows = rows[:100]
        ref = C.half_sqnorm_ref(rows)
        f32 = np.float32(0.5) * (rows[:, ::-1] * rows[:, ::-1]).sum(1, dtype=np.float32)     # another order, all in f32
        C.check_half_sqnorms(f32, rows)
        assert np.array_equal(C.ref_half_bits(rows, dtype), C.ref_half_bits(C.half_bits_to_f64(C.ref_half_bits(rows, dtype), dtype), dtype))
        assert np.array_equal(C.half_bits_to_f64(C.ref_half_bits(rows, dtype), dtype), rows), "the storage type holds the rows exactly"
        d_used = int(np.flatnonzero(np.abs(rows).sum(0))[-1]) + 1
        wrong = C.half_sqnorm_ref(rows[:, : d_used - 8])                                   # drops the last 8 columns
        if not name.startswith("int") or rows.shape[0] > 1:
            with pytest.raises(AssertionError):
                C.check_half_sqnorms(wrong, rows)
        assert np.isfinite(ref).all()
    sub = C.subnormal_rows()
    C.check_half_sqnorms(C.half_sqnorm_ref(sub), sub)
    with pytest.raises(AssertionError):
        C.check_half_sqnorms(np.zeros(sub.shape[0], np.float32), sub)                      # flushed subnormals


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_centroid_cases(dtype):
    for n, d, dim in C.CENTROID_CASES:
        rows = C.centroid_rows(n, d, dim, dtype)
        assert np.array_equal(C.half_bits_to_f64(C.ref_half_bits(rows, dtype), dtype), rows)
        ref = C.centroid_ref(rows, d)
        C.check_centroid_exact(ref, rows, d)
        if n > 1:
            with pytest.raises(AssertionError):
                C.check_centroid_exact(C.centroid_ref(rows[:-1], d) * np.float32((n - 1) / n), rows, d)
        bad = ref.copy()
        bad[dim - 1] = 1e-30
        if d < dim:
            with pytest.raises(AssertionError):
                C.check_centroid_exact(bad, rows, d)


def test_screen_check_accepts_the_model_and_rejects_a_skipped_row():
    for dim in (128, 768):
        n, dim8 = 9, C.screen_dim8(dim)
        for i, (row, col) in enumerate(C.positions(n, dim)):
            row_e = C.outlier_rows(n)[(i + 1) % 4]
            x = C.screen_corpus(n, dim, row, col, row_e, nan_before=bool(i % 2))
            x8, stats = C.screen_model(x, dim8)
            assert stats[0] == C.AMAX and stats[1] > dim / 5 and stats[2] > C.AMAX ** 2
            C.check_screen(x, x8, stats)
            if n - 1 in (row, row_e):
                with pytest.raises(AssertionError):
                    C.check_screen(x, *C.screen_model(x, dim8, skip_last_row=True))
            x8[1, dim8 - 1 if dim8 > dim else 0] += 3      # (row 1 is neither a deciding nor a NaN row)
            with pytest.raises(AssertionError):
                C.check_screen(x, x8, stats)


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_faithful_check_rejects_skipped_rows_and_columns(dtype):
    for d in C.FAITHFUL_DIMS:
        n = 9
        for row, col in C.positions(n, d, C.FAITHFUL_COLS):
            xf, xh = C.faithful_corpus(n, d, row, col, dtype, nan_before=True)
            ref = C.faithful_model(xf, xh)
            assert all(np.isfinite(ref)) and ref[0] > 0.1 and ref[1] > 1000
            up = np.array([C._f32_up(v) for v in ref], np.float32)
            C.check_faithful_stats(up, xf, xh)
            with pytest.raises(AssertionError, match="under-reported"):
                C.check_faithful_stats(np.nextafter(np.array(ref, np.float32), np.float32(0)), xf, xh)
            with pytest.raises(AssertionError, match="too loose"):
                C.check_faithful_stats(up * np.float32(1 + 2.0 ** -21), xf, xh)
            if row == n - 1:      # maxima that skip the last row
                with pytest.raises(AssertionError, match="under-reported"):
                    C.check_faithful_stats([C._f32_up(v) for v in C.faithful_model(xf, xh, rows=slice(0, n - 1))], xf, xh)
            if col >= 64 * (d // 64):      # maxima that skip the columns past the last multiple of 64
                with pytest.raises(AssertionError, match="under-reported"):
                    C.check_faithful_stats([C._f32_up(v) for v in C.faithful_model(xf, xh, cols=slice(0, 64 * (d // 64)))], xf, xh)
    xf, xh = C.faithful_corpus(9, 100, 4, 0, "fp16", overflow_row=6)
    assert np.isinf(xh[6]).sum() == 1 and C.faithful_model(xf, xh)[0] == np.inf
    C.check_faithful_stats(np.array([np.inf, C._f32_up(C.faithful_model(xf, xh)[1]), np.inf], np.float32), xf, xh)
    with pytest.raises(AssertionError, match="under-reported"):
        C.check_faithful_stats(np.array([3e38, 1200, np.inf], np.float32), xf, xh)
