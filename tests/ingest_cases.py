"""Generators, references and assertion helpers of the ingest and proof-build kernel tests: rr_rows_to_half, rr_l2_normalize_f32,
rr_half_sqnorms, rr_centroid, rr_screen_build and rr_faithful_build against plain numpy references (tests/test_ingest_gpu.py,
tests/test_proof_stats_gpu.py).  Importable without a GPU: tests/test_ingest_refs.py runs every check_* helper below on numpy
stand-ins of a right and of a subtly wrong kernel, so each check is known to pass and known to be able to fail.

Every tolerance is derived (U = 2^-24, the unit roundoff of f32), none is measured:
  conversion      bit for bit against numpy (fp16) / torch on the CPU (bf16), both round to nearest-even; NaN in = NaN out
  normalisation   (d/2 + 4) U relative per element: the f32 sum of d squares in any order is within d U, the square root halves
                  that; one rounding each for sqrtf, the reciprocal and the product, one U of slack for second-order terms
  sqnorms, centroid   bit for bit on data whose sums are exact in every order (integers below 2^24 times one power of two)
  screen stats    amax exactly; |x8 - x/s| <= 1/2 + 2^-20 |x/s|; the two row maxima within (dim + 8) U of the f64 sums
  faithful stats  never below ref (1 - d 2^-52), at most one f32 step above the upward rounding of ref (1 + d 2^-52)"""
import numpy as np

from tests.util import EXACT_CAP

U = 2.0 ** -24
DTYPES = ("fp16", "bf16")
RR_DTYPE = {"fp16": 0, "bf16": 1}
PASS_ROWS = 32768               # rows one grid-stride pass of the row kernels covers (8192 workgroups of 4 waves)
BIG_N = PASS_ROWS + 5
SENTINEL = 0x7B                 # every byte of an output buffer before the call; 0x7B7B is a finite non-zero fp16 and bf16
_FMT = {"fp16": (10, -14, 0x7C00, 0x03FF), "bf16": (7, -126, 0x7F80, 0x007F)}   # mantissa bits, least normal exponent, masks


def torch_dtype(dtype):
    import torch
    return torch.float16 if dtype == "fp16" else torch.bfloat16


# ---- 1. conversion -----------------------------------------------------------------------------------------------------------------
def _shuffled(v, seed):
    return np.ascontiguousarray(v[np.random.default_rng(seed).permutation(v.size)], dtype=np.float32)


def fp16_stream():
    """f32 inputs that pin f32 -> fp16: all 65 536 half patterns widened; for every adjacent pair of finite halves the exact
    midpoint and its two f32 neighbours (0 | 2^-24 gives 2^-25); 65504, 65520 (the overflow tie) and its neighbours; FLT_MAX, inf,
    0 and f32 subnormals; all of it in both signs.  Shuffled (fixed seed), so that every row of a layout mixes the classes."""
    every = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    mags = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)          # 0 ... 65504, ascending
    mid64 = (mags[:-1] + mags[1:]) / 2
    mid = mid64.astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), mid64)                                 # 12 significant bits: exact in f32
    inf = np.float32(np.inf)
    edge = np.array([65504, 65520, 2.0 ** -25, np.finfo(np.float32).max, np.inf, 0], np.float32)
    edge = np.concatenate([edge, np.nextafter(edge[1:3], 0), np.nextafter(edge[1:3], inf),
                           np.array([1, 2, 0x400000, 0x7FFFFF], np.uint32).view(np.float32)])
    pos = np.concatenate([np.nextafter(mid, np.float32(0)), mid, np.nextafter(mid, inf), edge])
    return _shuffled(np.concatenate([every, pos, -pos]), 16)


def bf16_stream():
    """Every 16-bit upper half of an f32 with the lower halves 0x0000 (exact), 0x0001, 0x7FFF (just below the tie), 0x8000 (the tie),
    0x8001 and 0xFFFF: every bf16 value, every tie with an even and with an odd upper neighbour, NaNs, infinities, f32 subnormals."""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    lo = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32)
    return _shuffled((hi[:, None] | lo[None, :]).reshape(-1).view(np.float32), 17)


def stream(dtype):
    return fp16_stream() if dtype == "fp16" else bf16_stream()


def lay_rows(vals, d, ld, n=None, gap=np.float32(-7777.0)):
    """(flat, x): x [n, d] filled from vals (cyclically) and the flat f32 buffer of EXACTLY (n - 1) ld + d floats that holds its rows
    ld apart; the floats between rows are `gap`, which no conversion may pick up."""
    if n is None:
        n = -(-vals.size // d)
    x = np.resize(vals, n * d).reshape(n, d)
    flat = np.full((n - 1) * ld + d, gap, np.float32)
    flat[np.arange(n, dtype=np.int64)[:, None] * ld + np.arange(d)[None, :]] = x
    return flat, x


def ref_half_bits(x, dtype):
    """uint16 patterns of round-to-nearest-even: numpy for fp16, torch on the CPU for bf16."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "fp16":
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            return x.astype(np.float16).view(np.uint16)
    import torch
    return torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def half_bits_to_f64(bits, dtype):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "fp16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def is_nan_bits(bits, dtype):
    _, _, e, m = _FMT[dtype]
    return ((bits & e) == e) & ((bits & m) != 0)


def check_half_bits(got, x, dtype):
    """got (uint16 patterns) is the nearest-even conversion of x: NaN exactly where x is NaN (payload free), every other pattern
    equal, the sign of zero included."""
    x = np.asarray(x, np.float32)
    ref = ref_half_bits(x, dtype)
    got = np.asarray(got).view(np.uint16).reshape(ref.shape)
    nan = np.isnan(x)
    assert np.array_equal(is_nan_bits(got, dtype), nan), "NaN in must give NaN out, and nothing else may"
    bad = (got != ref) & ~nan
    if bad.any():
        i = np.flatnonzero(bad.reshape(-1))[:8]
        raise AssertionError(f"{int(bad.sum())} of {bad.size} {dtype} conversions differ from nearest-even; first (f32 bits, got, want): "
                             + ", ".join(f"({b:#010x}, {g:#06x}, {w:#06x})" for b, g, w in
                                         zip(x.reshape(-1).view(np.uint32)[i], got.reshape(-1)[i], ref.reshape(-1)[i])))


def _f64(x):
    with np.errstate(invalid="ignore"):      # (the streams hold signalling NaNs)
        return np.asarray(x, np.float32).astype(np.float64)


def _quantum(a64, dtype):
    """Spacing of the half type's values around |x| (f64, exact powers of two)."""
    p, emin, _, _ = _FMT[dtype]
    with np.errstate(invalid="ignore"):
        e = np.frexp(np.where(np.isfinite(a64), a64, 1.0))[1] - 1
    return np.ldexp(1.0, np.maximum(e, emin) - p)


def _bits_of_exact(y64, dtype):
    """Patterns of f64 values that ARE values of the half type (or beyond its range: infinity)."""
    with np.errstate(over="ignore", invalid="ignore"):
        if dtype == "fp16":
            return y64.astype(np.float16).view(np.uint16)
        return (y64.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def convert_truncate(x, dtype):
    """A WRONG converter: rounds toward zero."""
    x64 = _f64(x)
    q = _quantum(np.abs(x64), dtype)
    with np.errstate(invalid="ignore"):
        return _bits_of_exact(np.copysign(np.floor(np.abs(x64) / q) * q, x64), dtype)


def convert_half_up(x, dtype):
    """A WRONG converter: rounds to nearest, ties away from zero."""
    x64 = _f64(x)
    q = _quantum(np.abs(x64), dtype)
    with np.errstate(invalid="ignore"):
        return _bits_of_exact(np.copysign(np.floor(np.abs(x64) / q + 0.5) * q, x64), dtype)


def tie_parities(x, dtype):
    """(even, odd): how many values of x lie exactly midway between two neighbouring values of the half type whose UPPER neighbour (in
    magnitude) has an even / an odd mantissa.  Nearest-even goes up on the first kind and down on the second; truncation is wrong on
    the first, ties-away on the second."""
    a = np.abs(_f64(x))
    fin = np.isfinite(a)
    a = np.where(fin, a, 0.0)
    q = _quantum(a, dtype)
    k = np.floor(a / q)
    tie = fin & ((a - k * q) * 2 == q)
    return int((tie & ((k + 1) % 2 == 0)).sum()), int((tie & ((k + 1) % 2 == 1)).sum())


# ---- 2. normalisation --------------------------------------------------------------------------------------------------------------
def normal_rows(rng, n, d):
    return (rng.standard_normal((n, d)) * 3).astype(np.float32)


def dominant_rows(rng, n, d):
    """One dominant element per row, every other element 2^-10 of it (random signs): an absolute tolerance sized for the dominant
    element hides any relative error of the rest."""
    a = (rng.uniform(1, 2, size=(n, 1)) * np.exp2(rng.integers(-6, 7, size=(n, 1)))).astype(np.float32)
    x = a * np.float32(2.0 ** -10) * rng.choice([-1, 1], size=(n, d)).astype(np.float32)
    x[np.arange(n), rng.integers(0, d, size=n)] = a[:, 0] * rng.choice([-1, 1], size=n).astype(np.float32)
    return x


def normalize_bound(d):
    return (d / 2 + 4) * U


def normalize_ref(x):
    x64 = np.asarray(x, np.float32).astype(np.float64)
    return x64 / np.sqrt((x64 * x64).sum(1, keepdims=True))


def check_normalized_f32(got, x):
    ref = normalize_ref(x)
    err = np.abs(np.asarray(got, np.float32).astype(np.float64) - ref)
    tol = normalize_bound(x.shape[1]) * np.abs(ref)
    bad = ~(err <= tol)
    assert not bad.any(), (f"{int(bad.sum())} elements outside (d/2 + 4) u relative; worst error / bound "
                           f"{float(np.nanmax(err / np.maximum(tol, 1e-300))):.3f}")


def _round_f64(v, dtype, toward):
    """Nearest-even rounding of f64 values to the half type, as f64.  fp16: numpy rounds f64 -> f16 once.  bf16 goes through f32,
    which is first moved outward (toward = -1 down, +1 up), so that the double rounding can only widen the interval."""
    if dtype == "fp16":
        with np.errstate(over="ignore", under="ignore"):
            return v.astype(np.float16).astype(np.float64)
    f = v.astype(np.float32)
    out = np.float32(np.inf) * toward
    f = np.where((f.astype(np.float64) - v) * toward < 0, np.nextafter(f, out), f).astype(np.float32)
    return half_bits_to_f64(ref_half_bits(f, "bf16"), "bf16")


def check_normalized_half(got_bits, x, dtype):
    """The stored half lies in [RNE(lo), RNE(hi)] of the interval ref (1 -+ (d/2 + 4) u), ends included."""
    ref = normalize_ref(x)
    w = normalize_bound(x.shape[1]) * np.abs(ref)
    lo, hi = _round_f64(ref - w, dtype, -1), _round_f64(ref + w, dtype, +1)
    g = half_bits_to_f64(np.asarray(got_bits).view(np.uint16).reshape(ref.shape), dtype)
    bad = ~((g >= lo) & (g <= hi))
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} {dtype} values outside [RNE(lo), RNE(hi)]"


EDGE_ROWS = ("zero", "squares underflow", "holds a NaN", "squares overflow")


def edge_rows(d):
    """[4, d] f32, one non-zero magnitude per row so that no summation order matters: all zero; +-2^-80 (every square underflows to
    zero: unchanged); 3 with one NaN (unchanged); +-2^70 (the sum of squares is +inf, 1 / inf = 0: the row becomes zeros)."""
    sign = np.where(np.arange(d) % 3 == 1, -1.0, 1.0).astype(np.float32)
    x = np.stack([np.zeros(d, np.float32), sign * np.float32(2.0 ** -80), np.full(d, 3, np.float32), sign * np.float32(2.0 ** 70)])
    x[2, d // 2] = np.nan
    return x


def edge_rows_expected(d):
    """What faiss' f32 arithmetic (oracle.normalize_L2) makes of edge_rows(d); the oracle's result is asserted to be the stated one."""
    from oracle import oracle as O
    x = edge_rows(d)
    want = x.copy()
    O.normalize_L2(want)
    assert np.array_equal(want[:3].view(np.uint32), x[:3].view(np.uint32)), "zero, underflowing and NaN rows stay unchanged"
    assert (want[3] == 0).all(), "a row whose sum of squares overflows becomes zeros"
    return x, want


def check_bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    v = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = got.view(v) != want.view(v)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ bit for bit; first at {np.argwhere(bad)[:4].tolist()}"


# ---- 3. |x|^2 / 2 of stored rows ---------------------------------------------------------------------------------------------------
SQNORM_DIMS = (128, 768, 1536, 8192)


def assert_exact_sqnorm(rows, exp=0):
    """The precondition of a bit-for-bit norm: every value is an integer times 2^exp and the row's sum of squares, in units of
    2^(2 exp), is below 2^24 - so is every partial sum in every order (the terms are non-negative), and f32 equals f64."""
    v = np.asarray(rows, np.float32).astype(np.float64) * 2.0 ** -exp
    assert np.array_equal(v, np.rint(v)), "values are not integers times 2^exp"
    assert (v * v).sum(1).max() < 1 << 24, "a row's sum of squares reaches 2^24: its f32 sum would depend on the order"


def pad_rows(x, dim):
    out = np.zeros((x.shape[0], dim), np.float32)
    out[:, : x.shape[1]] = x
    return out


def sqnorm_cases(dtype):
    """(name, rows f32 [n, dim] of values the storage type holds exactly, exp) - exact_case's l2 family and int_data at every dim and
    n, 32 768 + 5 rows at dim 128."""
    from tests.util import exact_case, int_data
    out = []
    for dim, n in [(dim, n) for dim in SQNORM_DIMS for n in (1, 5)] + [(128, BIG_N)]:
        rng = np.random.default_rng(1000 * dim + n)
        d = dim if dim != 768 else 700          # a zero-padded tail, as an index of d = 700 stores it
        out.append((f"l2-{dim}-{n}", pad_rows(exact_case(rng, n, 1, d, "l2", dtype)[0], dim), 0))
        out.append((f"int-{dim}-{n}", pad_rows(int_data(rng, n, d), dim), 0))
    for name, rows, exp in out:
        assert_exact_sqnorm(rows, exp)
    return out


def subnormal_rows(dim=128, n=5):
    """fp16 rows m 2^-24, |m| <= 300 with one +-1023 per row: every stored value subnormal, 127 * 300^2 + 1023^2 < 2^24."""
    rng = np.random.default_rng(24)
    m = rng.integers(-300, 301, size=(n, dim))
    m[np.arange(n), rng.integers(0, dim, size=n)] = 1023 * rng.choice([-1, 1], size=n)
    rows = (m.astype(np.float64) * 2.0 ** -24).astype(np.float32)
    assert_exact_sqnorm(rows, -24)
    assert np.abs(rows).max() < 2.0 ** -14
    return rows


def half_sqnorm_ref(rows):
    with np.errstate(over="ignore"):
        return (0.5 * (np.asarray(rows, np.float32).astype(np.float64) ** 2).sum(1)).astype(np.float32)


def check_half_sqnorms(got, rows):
    check_bits_equal(np.asarray(got, np.float32), half_sqnorm_ref(rows), "|x|^2 / 2")


# ---- 4. centroid -------------------------------------------------------------------------------------------------------------------
CENTROID_CASES = [(1, 64, 128), (777, 100, 128), (5000, 768, 768), (300, 4000, 4096), (300, 8192, 8192), (BIG_N, 100, 128)]


def centroid_rows(n, d, dim, dtype):
    """Integer rows [n, dim] (zero past d) whose column sums, and every partial sum of them, stay below 2^24: the float atomics of
    the kernel then commute."""
    amp = min(EXACT_CAP[dtype], ((1 << 24) - 1) // n)
    assert amp >= 1 and n * amp < 1 << 24
    rows = pad_rows(np.random.default_rng(n + d).integers(-amp, amp + 1, size=(n, d)).astype(np.float32), dim)
    assert np.abs(rows).sum(0).max() < 1 << 24
    return rows


def centroid_ref(rows, d):
    n, dim = rows.shape
    out = np.zeros(dim, np.float32)
    out[:d] = rows[:, :d].astype(np.float64).sum(0).astype(np.float32) * (np.float32(1) / np.float32(n))
    return out


def check_centroid_exact(got, rows, d):
    got = np.asarray(got, np.float32)
    assert (got[d:] == 0).all(), "entries d .. dim must be exactly zero"
    assert np.array_equal(got, centroid_ref(rows, d)), f"{int((got != centroid_ref(rows, d)).sum())} column means differ"


def check_centroid_close(got, rows, d):
    """Any data: within (n + 2) u mean|x| of the f64 mean per column (n additions in any order, the reciprocal, the product)."""
    r64 = rows[:, :d].astype(np.float64)
    err = np.abs(np.asarray(got, np.float32)[:d].astype(np.float64) - r64.mean(0))
    assert (err <= (rows.shape[0] + 2) * U * np.abs(r64).mean(0)).all(), float(err.max())
    assert (np.asarray(got)[d:] == 0).all()


# ---- 5. int8 screening copy --------------------------------------------------------------------------------------------------------
SCREEN_DIMS = (128, 768, 896, 1536)
AMAX = 127.0        # the planted maximum: s = 127 * fl(1 / 127), within 2^-23 of 1, so the small-integer base rows quantise (nearly) exactly


def screen_dim8(dim):
    return -(-dim // 256) * 256


def screen_scale(amax):
    a = np.float32(amax)
    return a * (np.float32(1) / np.float32(127)) if a > 0 else np.float32(1)


def outlier_rows(n):
    return [0, 3, 4, n - 1] + ([PASS_ROWS - 1, PASS_ROWS] if n > PASS_ROWS else [])


def outlier_cols(dim, cols=(0, 7, 8, 511, 512)):
    return [c for c in cols if c < dim - 1] + [dim - 1]


def positions(n, dim, cols=(0, 7, 8, 511, 512)):
    """(row, col) pairs: every outlier row and every outlier column at least once."""
    r, c = outlier_rows(n), outlier_cols(dim, cols)
    return [(r[i % len(r)], c[i % len(c)]) for i in range(max(len(r), len(c)))]


def screen_corpus(n, dim, row, col, row_e, seed=5, nan_before=False):
    """Small integers; (row, col) holds AMAX, which decides max|x| and, through its row, max|x|^2; row_e holds j + 1/2 in every
    column (the values that quantise worst under s ~ 1) and decides max|x - s x8|^2.  nan_before: the rows directly before the two
    deciding rows hold NaNs."""
    assert row != row_e
    x = np.random.default_rng(seed).integers(-2, 3, size=(n, dim)).astype(np.float32)
    x[row_e] = np.resize(np.array([0.5, -1.5, 1.5, -0.5, 2.5], np.float32), dim)
    x[row, col] = AMAX
    if nan_before:
        for r in (row - 1, row_e - 1):
            if r >= 0 and r not in (row, row_e):
                x[r, :: 5] = np.nan
    return x


def screen_model(rows, dim8, skip_last_row=False):
    """numpy statement of rr_screen_build: (x8 [n, dim8], stats f32[3]).  skip_last_row: a WRONG build whose maxima miss the last row."""
    r = np.asarray(rows, np.float32)
    used = r[:-1] if skip_last_row else r
    with np.errstate(invalid="ignore"):
        amax = np.float32(np.nanmax(np.abs(used), initial=0))
        s = screen_scale(amax)
        q = np.clip(np.rint(np.nan_to_num(r * (np.float32(1) / s), nan=-127.0)), -127, 127)
        e2 = ((r.astype(np.float64) - np.float64(s) * q) ** 2).sum(1)
        n2 = (r.astype(np.float64) ** 2).sum(1)
    if skip_last_row:
        e2, n2 = e2[:-1], n2[:-1]
    x8 = np.zeros((r.shape[0], dim8), np.int8)
    x8[:, : r.shape[1]] = q.astype(np.int8)
    return x8, np.array([amax, np.nanmax(e2, initial=0), np.nanmax(n2, initial=0)], np.float32)


def check_screen(rows, x8, stats):
    """rows: the stored values as f32 [n, dim] (finite, or NaN in some rows); x8 int8 [n, dim8]; stats f32 [>= 3]."""
    r = np.asarray(rows, np.float32).astype(np.float64)
    n, dim = r.shape
    x8 = np.asarray(x8, np.int8)
    stats = np.asarray(stats, np.float32)
    fin = ~np.isnan(r).any(1)
    assert stats[0] == np.nanmax(np.abs(r)), f"stats[0] = {stats[0]!r}, max|x| = {np.nanmax(np.abs(r))!r}"
    s = np.float64(screen_scale(stats[0]))
    assert x8.min() >= -127, "int8 values must lie in [-127, 127]"
    assert not x8[:, dim:].any(), "int8 columns dim .. rr_screen_dim(dim) must be zero"
    q = x8[fin, :dim].astype(np.float64)
    t = r[fin] / s
    assert (np.abs(q - t) <= 0.5 + 2.0 ** -20 * np.abs(t)).all(), "an int8 value is not the nearest integer to x / s"
    for w, ref, what in ((stats[1], ((r[fin] - s * q) ** 2).sum(1).max(), "max |x - s x8|^2"), (stats[2], (r[fin] ** 2).sum(1).max(), "max |x|^2")):
        assert abs(np.float64(w) - ref) <= (dim + 8) * U * ref, f"{what}: stats word {w!r}, f64 reference {ref!r}"


# ---- 6. f32-faithful maxima --------------------------------------------------------------------------------------------------------
FAITHFUL_DIMS = (100, 768, 1000)
FAITHFUL_COLS = (0, 63, 64)


def faithful_corpus(n, d, row, col, dtype, seed=6, nan_before=False, overflow_row=None):
    """(xf f32 [n, d], xh f32 [n, d] = its nearest-even half copy).  Standard-normal rows; (row, col) holds 1000.3, whose rounding
    error (fp16 spacing 1/2, bf16 spacing 4) and magnitude decide all three maxima - a kernel that misses that row or that column
    under-reports each of them by far more than the bound allows."""
    xf = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    xf[row, col] = 1000.3
    if nan_before and row > 0:
        xf[row - 1, :: 7] = np.nan
    if overflow_row is not None:
        xf[overflow_row, d // 3] = 70000.0
    return xf, half_bits_to_f64(ref_half_bits(xf, dtype), dtype).astype(np.float32)


def faithful_model(xf, xh, rows=slice(None), cols=slice(None)):
    """f64 reference (Dmax, Xmax, X~max) over the rows without a NaN; rows / cols restrict it to what a WRONG kernel would visit."""
    x, h = np.asarray(xf, np.float32).astype(np.float64)[rows, cols], np.asarray(xh, np.float32).astype(np.float64)[rows, cols]
    keep = ~np.isnan(np.asarray(xf)[rows]).any(1)
    with np.errstate(over="ignore", invalid="ignore"):
        return tuple(float(np.sqrt((v[keep] ** 2).sum(1)).max(initial=0)) for v in (x - h, x, h))


def _f32_up(v):
    with np.errstate(over="ignore"):
        f = np.float32(v)
    return np.nextafter(f, np.float32(np.inf)) if np.float64(f) < v else f


def check_faithful_stats(stats, xf, xh):
    """Each word is an upper bound (under-reporting is the unsound direction) and at most one f32 step loose."""
    d = np.asarray(xf).shape[1]
    for w, ref, what in zip(np.asarray(stats, np.float32)[:3], faithful_model(xf, xh), ("Dmax", "Xmax", "X~max")):
        lo, hi = ref * (1 - d * 2.0 ** -52), np.nextafter(_f32_up(ref * (1 + d * 2.0 ** -52)), np.float32(np.inf))
        assert np.float64(w) >= lo, f"{what} under-reported: {w!r} < {ref!r}"
        assert w <= hi, f"{what} too loose: {w!r} > {hi!r}"


# ---- device helpers ----------------------------------------------------------------------------------------------------------------
class Guarded:
    """An output tensor that is a slice of a larger buffer: `guard` leading and trailing rows (elements of a vector), every byte of
    the whole buffer prefilled with SENTINEL.  check() asserts that the rows around the slice still hold it."""

    def __init__(self, shape, tdt, dev, guard=3):
        import torch
        self.g = guard
        self.buf = torch.empty((shape[0] + 2 * guard,) + tuple(shape[1:]), dtype=tdt, device=dev)
        self.buf.view(torch.uint8).fill_(SENTINEL)
        self.out = self.buf[guard: guard + shape[0]]

    def check(self):
        import torch
        torch.cuda.synchronize()
        for part in (self.buf[: self.g], self.buf[self.g + self.out.shape[0]:]):
            assert bool((part.contiguous().view(torch.uint8) == SENTINEL).all()), "a kernel wrote outside its output"

    def bits(self):
        """The slice as numpy uint16 patterns (half types)."""
        import torch
        return self.out.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def to_half_device(rows, dtype, dev):
    """Stored rows (f32 values the half type holds, NaN and inf included) as a device tensor of the storage type, converted on the
    HOST: the kernels that read stored rows are tested on their own, not behind rr_rows_to_half."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(torch_dtype(dtype)).to(dev)
