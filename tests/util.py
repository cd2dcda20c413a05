"""Shared helpers for the parity tests (oracle = checker, ragroute_amd = thing under test)."""
import numpy as np


def half_round(x, dtype="fp16"):
    """Round f32 values to the storage dtype and back, so oracle and GPU see identical inputs."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    t = t.to(torch.float16 if dtype == "fp16" else torch.bfloat16).to(torch.float32)
    return t.numpy()


def int_data(rng, n, d, lo=-2, hi=3):
    """Small-integer embeddings: every dot product is an exact f32 integer in any summation order,
    so GPU scores must equal the oracle's bit for bit and ties are plentiful."""
    return rng.integers(lo, hi, size=(n, d)).astype(np.float32)


# ---- exact wide-value data: every stored mantissa bit and the exponent range, still bit-exact -------------------------------------
# int_data's values lie in {-2 ... 2}: three bits of each operand reach the matrix cores, and they survive a round trip through bf16
# and fp8 e4m3, so a kernel that drops low mantissa bits or unpacks a fragment through the wrong type passes every int_data test.
# The families below are integer valued too, but use every significant bit of the storage type, scaled so that every intermediate of
# an f32 accumulation stays an integer below 2^24 (times ONE power of two per (query, row) pair): every summation order gives the
# same f32, which therefore equals the f64 oracle's score bit for bit.
EXACT_LIMIT = (1 << 24) - 1                      # |partial sum| <= Aq Ax d <= 2^24 - 1: an exact f32 integer
EXACT_CAP = {"fp16": 2047, "bf16": 255}         # largest odd-inclusive integer range of 11 / 8 significant bits
EXACT_FAMILIES = ("rows", "queries", "balanced", "scaled", "l2")


def assert_exact_bounds(aq, ax, d, metric="ip", dtype=None):
    """The precondition of every exact family: inner product Aq Ax d < 2^24; squared L2 4 A^2 d <= 2^23, under which |x|^2 / 2,
    q.x - |x|^2 / 2 in any accumulation order, its double and |q|^2 - ... are all exact f32 values (multiples of 1/2 below 2^23)."""
    aq, ax, d = int(aq), int(ax), int(d)
    assert aq >= 1 and ax >= 1 and d >= 1
    if dtype is not None:
        assert max(aq, ax) <= EXACT_CAP[dtype], f"amplitude {max(aq, ax)} needs more significant bits than {dtype} stores"
    if metric == "l2":
        assert 4 * max(aq, ax) ** 2 * d <= 1 << 23, f"4 A^2 d = {4 * max(aq, ax) ** 2 * d} > 2^23: L2 distances would round"
    else:
        assert aq * ax * d < 1 << 24, f"Aq Ax d = {aq * ax * d} >= 2^24: partial sums would round"


def exact_amplitudes(d, family, dtype):
    """(Aq, Ax): the query and row amplitudes of a family at width d (values are uniform integers in [-A, A]).
    rows: every mantissa bit of the corpus operand matters, queries in {-1, 0, 1}; queries: the roles swapped; balanced: both
    operands as wide as the 2^24 bound allows; scaled: the rows-wide amplitudes, every row and query then times its own power of
    two (exact_case); l2: Aq = Ax with 4 A^2 d <= 2^23."""
    import math
    cap = EXACT_CAP[dtype]
    if family in ("rows", "scaled"):
        aq, ax = 1, min(cap, EXACT_LIMIT // d)
    elif family == "queries":
        aq, ax = min(cap, EXACT_LIMIT // d), 1
    elif family == "balanced":
        aq = ax = min(cap, math.isqrt(EXACT_LIMIT // d))
    elif family == "l2":
        aq = ax = min(cap, math.isqrt((1 << 21) // d))
    else:
        raise ValueError(f"unknown family {family!r}")
    assert_exact_bounds(aq, ax, d, "l2" if family == "l2" else "ip", dtype)
    return aq, ax


def exact_data(rng, n, d, amp):
    """Uniform integers in [-amp, amp] as f32 [n, d].  amp d < 2^24 is the least any caller needs (the other operand in {-1, 0, 1});
    a pair of operands goes through exact_case / assert_exact_bounds."""
    assert_exact_bounds(1, amp, d)
    return rng.integers(-int(amp), int(amp) + 1, size=(n, d)).astype(np.float32)


def exact_exponents(amp, dtype):
    """(lo, hi): powers of two a row of integers in [-amp, amp] may be scaled by so that every nonzero stored value is NORMAL and
    finite in the storage type (fp16: 2^-14 <= |v| < 2^15; bf16 has f32's exponent range, +-30 keeps every product and sum far
    inside the f32 normal range)."""
    if dtype == "fp16":
        return -14, 15 - int(amp).bit_length()
    return -30, 30


def exact_parts(rng, n, nq, d, family, dtype):
    """(mb i64 [n, d], eb i64 [n, 1], mq i64 [nq, d], eq i64 [nq, 1]): integer mantissas and power-of-two exponents per row / query
    (all zero except in the scaled family); the data are mb 2^eb and mq 2^eq."""
    aq, ax = exact_amplitudes(d, family, dtype)
    mb = rng.integers(-ax, ax + 1, size=(n, d))
    mq = rng.integers(-aq, aq + 1, size=(nq, d))
    for m, a in ((mb, ax), (mq, aq)):       # every wide vector holds +-A at least once (the caps 2047 / 255 are odd, all bits set): at
        if a > 1 and m.shape[0]:            # d = 8 one query in 256 has no odd value otherwise, and a lost low bit cannot show on it
            m[np.arange(m.shape[0]), rng.integers(0, d, size=m.shape[0])] = a * rng.choice([-1, 1], size=m.shape[0])
    eb, eq = np.zeros((n, 1), np.int64), np.zeros((nq, 1), np.int64)
    if family == "scaled":
        eb = rng.integers(exact_exponents(ax, dtype)[0], exact_exponents(ax, dtype)[1] + 1, size=(n, 1))
        eq = rng.integers(exact_exponents(aq, dtype)[0], exact_exponents(aq, dtype)[1] + 1, size=(nq, 1))
    return mb, eb, mq, eq


def scaled_f32(m, e):
    """m 2^e as f32 (exact: |m| < 2^24 and the exponents stay far inside f32's range)."""
    return (np.asarray(m, np.float64) * np.exp2(e)).astype(np.float32)


def exact_case(rng, n, nq, d, family, dtype):
    """(xb f32 [n, d], xq f32 [nq, d]) of one family; metric "l2" for the l2 family, "ip" for the others.  scaled: row r times
    2^e_r and query q times 2^e_q - a score is an integer below 2^24 times 2^(e_r + e_q), still exact, and rows of very different
    magnitude compete in one ranking."""
    mb, eb, mq, eq = exact_parts(rng, n, nq, d, family, dtype)
    return scaled_f32(mb, eb), scaled_f32(mq, eq)


SUBNORMAL_EXP = -24    # fp16 values below 2^-13 are spaced 2^-24: m 2^-24 is subnormal for |m| <= 1023, normal from 1024 on


def subnormal_case(rng, n, nq, d):
    """fp16, inner product: (xb, xq, pure) with rows m 2^-24.  `pure` rows (4 of 5) have |m| <= 1023: every stored value is an fp16
    SUBNORMAL; the others have |m| <= 1200, mostly subnormals with some values of the lowest normal binade, so that the ranking
    crosses the boundary.  Queries are {-1, 0, 1} times one power of two each.  A score is an integer (|.| <= 1200 d < 2^24) times a
    power of two: exact in any order - unless the hardware flushes subnormal inputs."""
    assert 1200 * d < 1 << 24
    pure = rng.random(n) >= 0.2
    m = np.where(pure[:, None], rng.integers(-1023, 1024, size=(n, d)), rng.integers(-1200, 1201, size=(n, d)))
    xb = scaled_f32(m, SUBNORMAL_EXP)
    xq = scaled_f32(rng.integers(-1, 2, size=(nq, d)), rng.integers(-2, 9, size=(nq, 1)))
    return xb, xq, pure


# what a subtly wrong kernel would do to an operand's integer mantissas (tests/test_wide_values_data.py: the exact families notice
# every one of them, int_data none)
def drop_one_bit(m):
    """v -> 2 trunc(v / 2): one bit of amplitude less."""
    return 2 * np.trunc(np.asarray(m, np.float64) / 2)


def round_bf16(m):
    """8 significant bits (the identity on integers up to 256)."""
    return half_round(np.asarray(m, np.float32), "bf16").astype(np.float64)


def round_e4m3(m):
    """fp8 e4m3: 4 significant bits, round to nearest even, saturating at 448 (the identity on integers up to 16)."""
    f, e = np.frexp(np.asarray(m, np.float64))
    return np.clip(np.ldexp(np.round(f * 16) / 16, e), -448, 448)


def clear_low_mantissa_bit(x, dtype):
    """Clear the lowest STORED mantissa bit of every value's fp16 / bf16 encoding: what a kernel does that masks an operand load
    or unpacks a fragment one bit short.  Invisible on int_data (its values have that bit clear), and on any value that does not use
    all 11 / 8 significant bits."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float16 if dtype == "fp16" else torch.bfloat16)
    return (t.view(torch.int16) & ~1).view(t.dtype).to(torch.float32).numpy()


def flush_fp16_subnormals(x):
    return np.where(np.abs(x) < 2.0 ** -14, np.float32(0), x).astype(np.float32)


def assert_topk_close(D, I, Dref, Iref, S=None, tol=1e-3):
    """Tolerance-aware parity: scores within tol position by position; ids identical wherever the
    oracle's ranking is unambiguous at tol (neighbouring gaps > 2*tol), and otherwise every returned
    id must be a legitimate member (its oracle score within tol of the position's score)."""
    assert D.shape == Dref.shape and I.shape == Iref.shape
    fin = np.isfinite(Dref)
    assert np.array_equal(np.isfinite(D), fin)
    assert np.allclose(D[fin], Dref[fin], atol=tol, rtol=0), float(np.abs(D[fin] - Dref[fin]).max())
    assert np.array_equal(I[~fin], Iref[~fin])
    nq, k = I.shape
    bad = 0
    for q in range(nq):
        if np.array_equal(I[q], Iref[q]):
            continue
        for j in range(k):
            if I[q, j] == Iref[q, j]:
                continue
            # ambiguous only if a neighbour of the oracle's position j is within 2*tol
            lo = Dref[q, j - 1] if j > 0 else np.inf
            hi = Dref[q, j + 1] if j + 1 < k else (-np.inf if S is None else np.partition(S[q], -k - 1)[-k - 1] if S.shape[1] > k else -np.inf)
            near = (lo - Dref[q, j] <= 2 * tol) or (Dref[q, j] - hi <= 2 * tol)
            assert near, f"query {q} pos {j}: id {I[q, j]} != {Iref[q, j]} with unambiguous oracle gap"
            if S is not None:
                assert abs(S[q, I[q, j]] - D[q, j]) <= tol
            bad += 1
    return bad


def tie_report(I, If, Df):
    """How FAISS orders EQUAL scores against this build's rule (ascending row id, include/ragroute_hip.h rr_flat_search): per query, the
    returned id SET (which rows make it past a tie at the k-th score) and the ORDER inside runs of equal scores."""
    set_same = all(set(a.tolist()) == set(b.tolist()) for a, b in zip(I, If))
    order_same = bool(np.array_equal(I, If))
    runs = asc = 0
    for q in range(If.shape[0]):
        j = 0
        while j < If.shape[1]:
            e = j
            while e + 1 < If.shape[1] and Df[q, e + 1] == Df[q, j]:
                e += 1
            if e > j:
                runs += 1
                asc += int(np.all(np.diff(If[q, j:e + 1]) > 0))
            j = e + 1
    return {"ties_set_identical": bool(set_same), "ties_order_identical": order_same, "tie_runs_in_faiss_result": runs,
            "faiss_tie_runs_in_ascending_id_order": asc}



# ---- synthetic router cases (shared by tests/golden/make_golden.py and the tests) -----------------
def synth_router_case(dataset, seed, n_queries=8):
    """Seeded synthetic router: state_dict, centroids, scaler statistics and query embeddings with the
    reference's shapes (router.py:32-34, config.py:32-101).  numpy's PCG64 stream is version-stable, so
    only the seed and the expected outputs need to be stored as fixtures."""
    from ragroute_amd import config as C
    rng = np.random.default_rng(seed)
    d_max = C.EMBEDDING_MAX_LENGTH[dataset]
    sources = C.DATA_SOURCES[dataset]
    n_in = C.ROUTER_INPUT_DIMENSION[dataset]
    u = lambda shape, b: rng.uniform(-b, b, size=shape).astype(np.float32)  # noqa: E731
    sd = {"fc1.weight": u((256, n_in), 3.0 / np.sqrt(n_in)), "fc1.bias": u((256,), 0.1),
          "ln1.weight": (1 + 0.2 * rng.standard_normal(256)).astype(np.float32), "ln1.bias": u((256,), 0.2),
          "fc2.weight": u((128, 256), 2.0 / 16), "fc2.bias": u((128,), 0.1),
          "ln2.weight": (1 + 0.2 * rng.standard_normal(128)).astype(np.float32), "ln2.bias": u((128,), 0.2),
          "fc3.weight": u((1, 128), 0.3), "fc3.bias": u((1,), 0.05)}
    model_dims = {}
    for s in sources:
        m = C.EMBEDDING_MODELS_PER_DATA_SOURCE[dataset][s][0]
        if m not in model_dims:
            model_dims[m] = d_max if dataset != "feb4rag" else int(rng.choice([768, 1024, 4096]))
    centroids = {}
    for s in sources:
        dm = model_dims[C.EMBEDDING_MODELS_PER_DATA_SOURCE[dataset][s][0]]
        centroids[s] = (0.5 * rng.standard_normal(dm)).astype(np.float32)
    scaler = None
    if dataset in ("medrag", "wikipedia"):
        scaler = (0.1 * rng.standard_normal(n_in), rng.uniform(0.5, 2.0, size=n_in))
    queries = [{m: rng.standard_normal(dm).astype(np.float32) for m, dm in model_dims.items()} for _ in range(n_queries)]
    return {"dataset": dataset, "sources": sources, "sd": sd, "centroids": centroids, "scaler": scaler, "queries": queries,
            "d_max": d_max}


def synth_medrag_corpus(seed, n=600, d=768):
    """Small integer-valued 'pubmed'-shaped data source: rows, metadatas (row -> {index, source}) and chunk files."""
    rng = np.random.default_rng(seed)
    xb = int_data(rng, n, d)
    books = ["bookA", "bookB", "bookC"]
    per = n // len(books)
    metadatas = [{"index": i % per, "source": books[min(i // per, len(books) - 1)]} for i in range(n)]
    chunks = {b: [{"id": f"{b}_{j}", "title": f"title {b} {j}", "content": f"content of {b} chunk {j}"} for j in range(per + n)] for b in books}
    return xb, metadatas, chunks


def flat_golden_inputs(case):
    """Seeded inputs of the flat-search fixture tests/golden/flat_search.npz (N=4096, d=768, B=8, k=32,
    fp16-rounded).  Only the expected outputs are stored; the inputs are regenerated from the seed (numpy's PCG64 streams
    are stable across versions)."""
    rng = np.random.default_rng({"gauss": 101, "int": 102, "cosine": 103}[case])
    n, d, nq = 4096, 768, 8
    if case == "int":
        return int_data(rng, n, d), int_data(rng, nq, d)
    xb = rng.standard_normal((n, d)).astype(np.float32)
    xq = rng.standard_normal((nq, d)).astype(np.float32)
    if case == "cosine":   # normalise in f64, then round to the stored precision: what the index holds
        xb = (xb / np.linalg.norm(xb.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
        xq = (xq / np.linalg.norm(xq.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    else:
        xb /= np.float32(np.sqrt(d))
    return half_round(xb), half_round(xq)
