"""CPU: the exact wide-value data of tests/util.py (exact_case, subnormal_case) are what tests/test_wide_values_gpu.py needs them
to be, at every (d, family, dtype) cell a GPU test uses (tests/wide_cases.py cells()):

  round trip          unchanged by a round trip through the storage type, every nonzero value normal and finite there;
  order independence  an f32 accumulation equals the f64 oracle's score bit for bit in ascending order, in a random order and as
                      blocks of 32 followed by a tree - every PREFIX of each order is checked against f64, not just the end;
                      for L2 the kernels' formula |q|^2 - 2 (q.x - |x|^2 / 2) in f32 equals the oracle's distance;
  sensitivity         what makes the GPU tests able to fail: a mutation of the wide operand (one bit of amplitude less, bf16 or
                      fp8 e4m3 rounding, the lowest stored mantissa bit cleared) changes the oracle's top-k for EVERY query;
  the gap, on record  the same roundings and the cleared mantissa bit leave int_data's results unchanged.

Where a mutation is the identity by construction it is not applied: bf16 rounding on amplitudes <= 256, e4m3 rounding on
amplitudes <= 16 (every integer up to there is representable), the cleared mantissa bit where the amplitude is below the storage
type's cap (no value uses the lowest bit of the encoding)."""
import numpy as np
import pytest

from tests import wide_cases as W
from tests.util import (EXACT_CAP, clear_low_mantissa_bit, drop_one_bit, exact_amplitudes, exact_case, exact_parts,
                        flush_fp16_subnormals, half_round, int_data, round_bf16, round_e4m3, scaled_f32, subnormal_case)

CELLS = W.cells()
N, NQ, K = 3000, 8, 10          # sensitivity: rows, queries, k
IDS = [f"{d}-{fam}-{dt}" for d, fam, dt in CELLS]


def _oracle(metric):
    from oracle import oracle as O
    return O.flat_search_l2 if metric == "l2" else O.flat_search_ip


def _metric(fam):
    return "l2" if fam == "l2" else "ip"


def _all_scores(xb, xq, metric):
    """The oracle's f32 score of every (query, row) pair, through its own search at k = n."""
    n = xb.shape[0]
    D, I = _oracle(metric)(xb, xq, n)
    S = np.empty_like(D)
    np.put_along_axis(S, I, D, axis=1)
    return S


def _orders(P, rng):
    """Final f32 sums of the products P [..., d] in three orders; asserts that every prefix of every order is exact (equal to the
    same prefix summed in f64)."""
    def seq(X):
        c32, c64 = np.cumsum(X, axis=-1, dtype=np.float32), np.cumsum(X.astype(np.float64), axis=-1)
        assert np.array_equal(c32.astype(np.float64), c64), "an f32 partial sum rounded"
        return c32[..., -1]
    d = P.shape[-1]
    out = [seq(P), seq(P[..., rng.permutation(d)])]
    pad = (-d) % 32
    B = np.concatenate([P, np.zeros(P.shape[:-1] + (pad,), np.float32)], axis=-1).reshape(P.shape[:-1] + (-1, 32))
    level = np.moveaxis(np.cumsum(B, axis=-1, dtype=np.float32)[..., -1], -1, 0)          # [blocks, ...]: 32 sequential adds each
    while level.shape[0] > 1:
        if level.shape[0] % 2:
            level = np.concatenate([level, np.zeros_like(level[:1])])
        s = level[0::2] + level[1::2]
        assert s.dtype == np.float32 and np.array_equal(s.astype(np.float64), level[0::2].astype(np.float64) + level[1::2])
        level = s
    out.append(level[0])
    return out


def test_the_cells_cover_what_the_gpu_tests_use():
    used = {(c["d"], c["family"], c["dtype"]) for c in W.flat_cases()} | W.fuzz_cells()
    used |= {(d, fam, dt) for d, _, _, _ in W.SEGMENT_CASES for pairs in W.SEGMENT_DATA.values() for fam, dt in pairs}
    used |= {(d, fam, dt) for d, _, _, _ in W.SCREEN_CASES for fam in W.IP_FAMILIES for dt in W.DTYPES}
    assert used == set(CELLS)
    assert {d for d, _, _ in W.fuzz_cells()} - {d for d, _ in W.GRID}, "the fuzz samples bring widths of their own"
    assert {d for d, _, _ in CELLS} >= {8, 100, 768, 769, 1536, 4096, 8192}
    assert {f for _, f, _ in CELLS} == set(W.FAMILIES) and {t for _, _, t in CELLS} == set(W.DTYPES)


def test_the_flat_cases_reach_all_five_scan_kernels_in_both_dtypes_and_modes():
    """The dispatch report needs no device: every kernel x (dense, chunked) x (fp16, bf16) x family, and no sixth kernel name."""
    from ragroute_amd import _lib
    reached = W.assert_kernel_coverage(_lib.lib())
    print({k: len(v) for k, v in reached.items()})


def test_amplitudes_are_the_documented_ones():
    assert exact_amplitudes(8192, "rows", "fp16") == (1, 2047) and exact_amplitudes(8192, "queries", "fp16") == (2047, 1)
    assert exact_amplitudes(768, "rows", "bf16") == (1, 255)
    assert [exact_amplitudes(d, "balanced", "fp16")[0] for d in (768, 4096, 8192)] == [147, 63, 45]
    assert [exact_amplitudes(d, "l2", "fp16")[0] for d in (768, 8192)] == [52, 16]
    assert exact_amplitudes(8, "balanced", "fp16") == (1448, 1448) and exact_amplitudes(8, "balanced", "bf16") == (255, 255)


def test_a_careless_caller_cannot_make_inexact_data():
    from tests.util import assert_exact_bounds, exact_data
    rng = np.random.default_rng(0)
    with pytest.raises(AssertionError):
        exact_data(rng, 4, 8192, 2048)                   # 2048 * 8192 = 2^24
    with pytest.raises(AssertionError):
        assert_exact_bounds(148, 148, 768)               # balanced + 1
    with pytest.raises(AssertionError):
        assert_exact_bounds(53, 53, 768, "l2")           # l2 + 1
    with pytest.raises(AssertionError):
        assert_exact_bounds(1, 256, 8, "ip", "bf16")     # nine significant bits
    with pytest.raises(AssertionError):
        subnormal_case(rng, 4, 2, 16_384)


@pytest.mark.parametrize("d,fam,dt", CELLS, ids=IDS)
def test_round_trip_through_the_storage_type(d, fam, dt):
    xb, xq = exact_case(np.random.default_rng(d), 512, 64, d, fam, dt)
    tiny, huge = (2.0 ** -14, 65504.0) if dt == "fp16" else (2.0 ** -126, 3.38e38)
    for x in (xb, xq):
        assert np.array_equal(half_round(x, dt), x)
        assert np.all((x == 0) | ((np.abs(x) >= tiny) & (np.abs(x) <= huge)))
    aq, ax = exact_amplitudes(d, fam, dt)
    if fam != "scaled":
        assert ax / 2 < np.abs(xb).max() <= ax and aq / 2 < np.abs(xq).max() <= aq     # the amplitude's top bit is in use
    else:                                                                  # rows of very different magnitude in one ranking
        assert np.ptp(np.log2(np.abs(xb).max(1))) >= 16


@pytest.mark.parametrize("d,fam,dt", CELLS, ids=IDS)
def test_f32_accumulation_is_order_independent_and_equals_the_oracle(d, fam, dt):
    rng = np.random.default_rng(d + 1)
    n, nq = (96, 4) if d <= 2048 else (32, 3)
    xb, xq = exact_case(rng, n, nq, d, fam, dt)
    S = _all_scores(xb, xq, _metric(fam))
    P = xq[:, None, :] * xb[None, :, :]
    assert P.dtype == np.float32 and np.array_equal(P.astype(np.float64), xq[:, None, :].astype(np.float64) * xb[None, :, :])
    if fam != "l2":
        for got in _orders(P, rng):
            assert np.array_equal(got, S)
        return
    # the kernels' L2 form: hn = |x|^2 / 2 (rr_half_sqnorms), rank by s = q.x - hn, D = |q|^2 - 2 s; the norm enters the sum first
    # (accumulator seeded with -hn) or last, in every order of the products
    dots = _orders(P, rng)
    for hn in _orders(xb * xb, rng):
        hn = hn * np.float32(0.5)
        assert np.array_equal(hn.astype(np.float64), 0.5 * (xb.astype(np.float64) ** 2).sum(1))
        for qq in _orders(xq * xq, rng):
            for dot in dots:
                assert np.array_equal(qq[:, None] - np.float32(2) * (dot - hn[None, :]), S)
            seeded = np.concatenate([np.broadcast_to(-hn[None, :, None], P.shape[:2] + (1,)), P], axis=-1)
            for s in _orders(seeded, rng)[:1]:
                assert np.array_equal(qq[:, None] - np.float32(2) * s, S)


def _differs_for_every_query(a, b):
    (Da, Ia), (Db, Ib) = a, b
    return bool(np.all((Da != Db).any(1) | (Ia != Ib).any(1)))


@pytest.mark.parametrize("d,fam,dt", CELLS, ids=IDS)
def test_a_mutated_wide_operand_changes_every_query(d, fam, dt):
    rng = np.random.default_rng(d + 2)
    mb, eb, mq, eq = exact_parts(rng, N, NQ, d, fam, dt)
    aq, ax = exact_amplitudes(d, fam, dt)
    amp, rows_wide = max(aq, ax), ax >= aq
    search = _oracle(_metric(fam))
    xb, xq = scaled_f32(mb, eb), scaled_f32(mq, eq)
    base = search(xb, xq, K)
    mutations = [("one bit of amplitude less", drop_one_bit)]
    if amp > 256:
        mutations.append(("bf16 rounding", round_bf16))
    if amp > 16:
        mutations.append(("fp8 e4m3 rounding", round_e4m3))
    for name, mut in mutations:
        got = search(scaled_f32(mut(mb), eb), xq, K) if rows_wide else search(xb, scaled_f32(mut(mq), eq), K)
        assert _differs_for_every_query(base, got), name
    if amp == EXACT_CAP[dt]:      # the lowest bit of the ENCODING is in use: a masked operand load shows
        got = search(clear_low_mantissa_bit(xb, dt), xq, K) if rows_wide else search(xb, clear_low_mantissa_bit(xq, dt), K)
        assert _differs_for_every_query(base, got), "lowest stored mantissa bit cleared"


@pytest.mark.parametrize("d", [100, 768, 4096])
def test_the_gap_int_data_notices_none_of_it(d):
    """int_data's values {-2 ... 2} survive bf16 and fp8 rounding and have the lowest stored mantissa bit clear in both storage types:
    a kernel that did any of that to an operand would still pass every int_data test.  (v -> 2 trunc(v / 2) is not in this list: it
    turns +-1 into 0, which int_data does notice; what int_data cannot see is the loss of LOW bits of a wide mantissa.)"""
    from oracle import oracle as O
    rng = np.random.default_rng(d)
    xb, xq = int_data(rng, N, d), int_data(rng, NQ, d)
    base = O.flat_search_ip(xb, xq, K)
    for mut in (round_bf16, round_e4m3, lambda x: clear_low_mantissa_bit(x, "fp16"), lambda x: clear_low_mantissa_bit(x, "bf16")):
        for got in (O.flat_search_ip(np.asarray(mut(xb), np.float32), xq, K), O.flat_search_ip(xb, np.asarray(mut(xq), np.float32), K)):
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])


@pytest.mark.parametrize("d", sorted({d for d, _ in W.SUBNORMAL_CASES}))
def test_subnormal_family(d):
    from oracle import oracle as O
    rng = np.random.default_rng(d)
    xb, xq, pure = subnormal_case(rng, N, NQ, d)
    assert np.array_equal(half_round(xb), xb) and np.array_equal(half_round(xq), xq)
    assert np.all(np.abs(xb[pure]) < 2.0 ** -14) and np.abs(xb[~pure]).max() >= 2.0 ** -14       # subnormal rows; rows that cross
    assert 0.5 < np.mean(np.abs(xb) < 2.0 ** -14) and np.mean(xb != 0) > 0.99
    S = _all_scores(xb[:64], xq[:3], "ip")
    for got in _orders(xq[:3, None, :] * xb[None, :64, :], rng):
        assert np.array_equal(got, S)
    base = O.flat_search_ip(xb, xq, K)
    assert all(pure[i].any() and not pure[i].all() for i in base[1]), "every query's top-k should hold rows of both kinds"
    assert _differs_for_every_query(base, O.flat_search_ip(flush_fp16_subnormals(xb), xq, K))
