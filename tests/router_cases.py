"""Inputs, reference, tolerance and wrong-kernel stand-ins of the router MLP kernel tests (csrc/router.hip: router_mlp_kernel, and
router_fc1_kernel + router_head_kernel on the matrix cores).  Plain numpy, importable without a GPU: tests/test_router_refs.py runs
every check on the CPU, tests/test_router_kernels_gpu.py runs the kernels against the same cases.

Reference.  folded_forward64 states the operator of include/ragroute_hip.h (rr_router_weights) in float64:
    fc1 = q_model(c) . W1q' + c1[c];  h1 = relu(LN256(fc1));  h2 = relu(LN128(h1 W2 + b2));  logit = h2 . w3 + b3
with LayerNorm's biased variance and eps inside the square root.  Nothing is folded here: the cases hand W1q' and c1 to the kernels
as they are (router.fold_weights has its own CPU tests).

Exact-fc1 family.  w1q holds integers in [-3, 3], queries integers in [-2, 2], c1 integers in [-8, 8] times one power of two per
case (plus an integer offset in one case); every fc1 product and partial sum is an integer (times that power of two) below 2^24, so
fc1 is exact in f32 in ANY summation order - the four k-quarters of the small kernel, the per-chunk partials of the matrix-core form
- and equals the float64 value (assert_exact_fc1).  A wrong column, chunk, row of c1 or embedding therefore shows at full size, and
all remaining error comes from the two LayerNorms, fc2 (256 terms) and fc3 (128 terms).  Every other tensor holds random f32 values.

Tolerance.  Measured from the reference alone: forward32 restates the same forward in f32 numpy with three summation orders of its
reductions (ascending, descending, numpy's pairwise); e32(case) is the largest deviation of any of them from folded_forward64 over
the case's rows, and the case's tolerance is MARGIN x e32.  The margin of 8 is there because the kernels' orders are none of the
three (64-lane butterflies, two interleaved fmaf chains or the matrix cores' K pairs in fc2).  Every case must satisfy
MARGIN x e32 <= LOGIT_TOL / 10 (tests/test_router_refs.py), so a tolerance that grows cannot hide a failure."""
import functools

import numpy as np

LOGIT_TOL = 2e-4                 # the bound of tests/test_router_merge_gpu.py, against the reference project's logits
MARGIN = 8
TOL_CAP = LOGIT_TOL / 10
LN_EPS = 1e-5
MASK_MARGIN = 1e-6               # p in (0, 1): an f32 expf, add and divide err by a few 2^-24 = 6e-8 each
NAN_LOGIT_BITS = 0x7FC0ABAB      # every f32 of an output buffer before the call (a NaN no kernel produces)
MASK_SENTINEL = 0xAB
# Every error of the head reaches the logit through w3, so e32 scales with it.  With w3 in +-0.3 (tests.util.synth_router_case) the
# worst of the strictly sequential f32 orders over a case's thousands of rows is 1.2 ... 2.8e-6, and 8 x that passes the 2e-5 cap on
# some cases and misses it on others; +-1/8 (logits of a few tenths) keeps every case a factor of two inside the cap.  The ratio
# between a wrong kernel's effect and the tolerance does not depend on this scale.
W3_RANGE = 0.125

DEFAULT_TOPOLOGY = (0, 0, 0, 0, 0, 1, 1, 1, 1)      # 9 sources on 2 models; model 0 serves 5 (more than the 4 wave slots)
RAGGED_TOPOLOGY = (0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 0, 0)   # 13 sources on 8 models
COLUMN_WIDTHS = (1, 4, 100, 128, 130, 132, 770)
RAGGED_NQ = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 96, 97, 129)
TAIL_STARTS = (0, 1, 127, 128, 129, 769)
MAX_DMAX = 8191


class Weights:
    """The tensors of rr_router_weights as numpy f32 arrays (w1q [d_max][256], c1 [C][256], w2 [256][128], ...)."""
    FIELDS = ("w1q", "c1", "ln1_g", "ln1_b", "w2", "b2", "ln2_g", "ln2_b", "w3")

    def __init__(self, model_of_source, n_models=None, b3=0.0, thr=0.5, eps=LN_EPS, **tensors):
        for f in self.FIELDS:
            setattr(self, f, np.ascontiguousarray(tensors[f], dtype=np.float32))
        self.model_of_source = np.asarray(model_of_source, np.int64)
        self.n_models = int(self.model_of_source.max()) + 1 if n_models is None else int(n_models)
        self.b3, self.thr, self.eps = np.float32(b3), np.float32(thr), np.float32(eps)
        self.d_max, self.n_sources = self.w1q.shape[0], self.c1.shape[0]
        assert self.w1q.shape == (self.d_max, 256) and self.c1.shape == (self.n_sources, 256) and self.w2.shape == (256, 128)
        assert len(self.model_of_source) == self.n_sources and self.model_of_source.max() < self.n_models

    def replace(self, **kw):
        d = {f: getattr(self, f) for f in self.FIELDS}
        d.update(model_of_source=self.model_of_source, n_models=self.n_models, b3=self.b3, thr=self.thr, eps=self.eps)
        d.update(kw)
        return Weights(**d)

    def state_dict(self):
        """The keys ragroute_amd.router.FoldedRouter reads (reference layout: fc2.weight [128][256], fc3.weight [1][128])."""
        return {"ln1.weight": self.ln1_g, "ln1.bias": self.ln1_b, "fc2.weight": self.w2.T, "fc2.bias": self.b2, "ln2.weight": self.ln2_g,
                "ln2.bias": self.ln2_b, "fc3.weight": self.w3[None, :], "fc3.bias": np.array([self.b3], np.float32)}


def exact_weights(seed, d_max, model_of_source, n_models=None, c1_exp=0, c1_offset=0, thr=0.5, zero_w1q=False, constant_c1=False):
    rng = np.random.default_rng(seed)
    C = len(model_of_source)
    u = lambda shape, b: rng.uniform(-b, b, size=shape).astype(np.float32)  # noqa: E731
    w1q = rng.integers(-3, 4, size=(d_max, 256))
    c1 = rng.integers(-8, 9, size=(C, 256))
    if zero_w1q:
        w1q[:] = 0
    if constant_c1:
        c1 = np.repeat(np.arange(-(C // 2), C - C // 2)[:, None], 256, axis=1)    # row c holds one value, every row another
    c1 = c1 * 2.0 ** c1_exp + c1_offset
    assert len({r.tobytes() for r in c1}) == C, "every c1 row distinct: a row of the wrong source must show"
    return Weights(model_of_source, n_models, b3=u((1,), 0.05)[0], thr=thr, w1q=w1q, c1=c1,
                   ln1_g=(1 + 0.2 * rng.standard_normal(256)), ln1_b=u((256,), 0.2), w2=u((256, 128), 2.0 / 16), b2=u((128,), 0.1),
                   ln2_g=(1 + 0.2 * rng.standard_normal(128)), ln2_b=u((128,), 0.2), w3=u((128,), W3_RANGE))


def int_queries(rng, nq, n_models, d_max):
    return rng.integers(-2, 3, size=(nq, n_models, d_max)).astype(np.float32)


def assert_exact_fc1(w, xq):
    """The precondition of the family: with g the common power-of-two quantum of c1 (at most 1), sum |x| |w| + |c1| < 2^24 g for
    every (query, source) row - every partial sum in every order is then a multiple of g below 2^24 g, an exact f32."""
    c1 = w.c1.astype(np.float64)
    g = 1.0
    while not np.array_equal(np.rint(c1 / g), c1 / g):
        g /= 2
        assert g > 2.0 ** -30
    for a in (w.w1q, xq[np.isfinite(xq)]):
        assert np.array_equal(np.rint(a), a), "w1q and the queries hold integers"
    reach = (np.abs(np.nan_to_num(xq)).astype(np.float64) @ np.abs(w.w1q).astype(np.float64)).max(initial=0) + np.abs(c1).max()
    assert reach < 2.0 ** 24 * g, f"fc1 partial sums reach {reach} at quantum {g}: they would round in f32"


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def _fc1_64(w, xq, model_of_source=None, c1=None):
    mos = w.model_of_source if model_of_source is None else np.asarray(model_of_source)
    with np.errstate(invalid="ignore"):
        u = np.einsum("qmd,dj->qmj", np.asarray(xq, np.float32).astype(np.float64), w.w1q.astype(np.float64))
    return u[:, mos, :] + (w.c1 if c1 is None else c1).astype(np.float64)[None]


def _ln64(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g.astype(np.float64) + b.astype(np.float64)


def _head64(w, fc1, ln1=_ln64, ln2=_ln64):
    eps = np.float64(w.eps)
    with np.errstate(invalid="ignore"):
        h1 = np.maximum(ln1(fc1, w.ln1_g, w.ln1_b, eps), 0)
        h2 = np.maximum(ln2(h1 @ w.w2.astype(np.float64) + w.b2.astype(np.float64), w.ln2_g, w.ln2_b, eps), 0)
        return h2 @ w.w3.astype(np.float64) + np.float64(w.b3)


def sigmoid64(logits):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)))


def folded_forward64(w, xq):
    """(logits f64 [nq][C], sigmoid f64 [nq][C]) of queries xq f32 [nq][n_models][d_max]."""
    logits = _head64(w, _fc1_64(w, xq))
    return logits, sigmoid64(logits)


def mask_of(w, logits):
    return sigmoid64(logits) > np.float64(w.thr)


# ---- the same forward in f32, three summation orders -----------------------------------------------------------------------------------
ORDERS = ("ascending", "descending", "pairwise")


def _rsum32(x, order):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if order == "pairwise":
        return x.sum(-1, dtype=np.float32)
    return np.cumsum(x if order == "ascending" else x[..., ::-1], axis=-1, dtype=np.float32)[..., -1]


def _ln32(x, g, b, eps, order):
    inv_n = np.float32(1) / np.float32(x.shape[-1])
    d = x - (_rsum32(x, order) * inv_n)[..., None]
    rstd = np.float32(1) / np.sqrt(_rsum32(d * d, order) * inv_n + eps)
    return np.maximum(d * rstd[..., None] * g + b, np.float32(0))


def forward32(w, xq, order):
    """logits f32 [nq][C]: fc1 exact (asserted), everything after it in f32 with the reductions taken in `order`."""
    fc1_64 = _fc1_64(w, xq)
    fc1 = fc1_64.astype(np.float32)
    assert np.array_equal(fc1.astype(np.float64), fc1_64), "fc1 of an exact-fc1 case is an f32 value"
    h1 = _ln32(fc1.reshape(-1, 256), w.ln1_g, w.ln1_b, w.eps, order)
    z = np.empty((h1.shape[0], 128), np.float32)
    if order == "pairwise":
        w2t = np.ascontiguousarray(w.w2.T)
        for r in range(0, h1.shape[0], 256):
            z[r:r + 256] = (h1[r:r + 256, None, :] * w2t[None]).sum(-1, dtype=np.float32)
    else:
        z[:] = 0
        for i in (range(256) if order == "ascending" else range(255, -1, -1)):
            z += h1[:, i:i + 1] * w.w2[i][None, :]
    h2 = _ln32(z + w.b2, w.ln2_g, w.ln2_b, w.eps, order)
    return (_rsum32(h2 * w.w3, order) + w.b3).reshape(fc1.shape[:2])


# ---- wrong kernels ---------------------------------------------------------------------------------------------------------------------
def _drop_columns(xq, keep):
    x = np.array(xq, np.float32)
    x[..., keep:] = 0
    return x


def _stop_at_query0(xq):
    """The small kernel's k loop ended at the last non-zero input of the FIRST query of each group of 4, not of the group."""
    x = np.array(xq, np.float32)
    for q0 in range(0, x.shape[0], 4):
        for m in range(x.shape[1]):
            nz = np.flatnonzero(x[q0, m])
            x[q0:q0 + 4, m, (nz[-1] + 1 if nz.size else 0):] = 0
    return x


def thread_last_kend(x4):
    """Where the small kernel's k loop ended before its fix: thread tid of 1024 visits the flattened [4][d_max] inputs of a group
    at tid, tid + 1024, ... and kept the column of the LAST non-zero input it saw, not of the furthest; the loop end is the
    maximum over the threads.  Equal to the true end while 4 d_max <= 1024 (one visit per thread)."""
    d = x4.shape[1]
    flat = np.zeros(-(-4 * d // 1024) * 1024, np.float32)
    flat[:x4.size] = x4.reshape(-1)
    nz = flat.reshape(-1, 1024) != 0                                  # [visit][tid]
    col = (np.arange(flat.size) % d + 1).reshape(-1, 1024)
    last_visit = nz.shape[0] - 1 - np.argmax(nz[::-1], axis=0)
    return int(np.where(nz.any(0), col[last_visit, np.arange(1024)], 0).max())


def _stop_at_thread_last(xq):
    x = np.array(xq, np.float32)
    for q0 in range(0, x.shape[0], 4):
        for m in range(x.shape[1]):
            x4 = np.zeros((4, x.shape[2]), np.float32)
            x4[:x[q0:q0 + 4].shape[0]] = x[q0:q0 + 4, m]
            x[q0:q0 + 4, m, thread_last_kend(x4):] = 0
    return x


def _ln_unbiased(x, g, b, eps):
    n = x.shape[-1]
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).sum(-1, keepdims=True) / (n - 1) + eps) * g + b


def _ln_eps_outside(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / (np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True)) + eps) * g + b


def _ln_one_pass_f32(x, g, b, eps):
    x32 = x.astype(np.float32)
    inv_n = np.float32(1) / np.float32(x.shape[-1])
    mu = x32.sum(-1, dtype=np.float32, keepdims=True) * inv_n
    var = np.maximum((x32 * x32).sum(-1, dtype=np.float32, keepdims=True) * inv_n - mu * mu, np.float32(0))
    return ((x32 - mu) / np.sqrt(var + np.float32(eps))).astype(np.float64) * g + b


STAND_INS = {
    "fc1 drops the last column": lambda w, xq: _head64(w, _fc1_64(w, _drop_columns(xq, w.d_max - 1))),
    "fc1 drops the columns past the last multiple of 128": lambda w, xq: _head64(w, _fc1_64(w, _drop_columns(xq, w.d_max // 128 * 128))),
    "fc1 drops the columns past the last multiple of 4": lambda w, xq: _head64(w, _fc1_64(w, _drop_columns(xq, w.d_max // 4 * 4))),
    "fc1 stops at the last non-zero input of query 0 of a group": lambda w, xq: _head64(w, _fc1_64(w, _stop_at_query0(xq))),
    "fc1 stops where a thread last saw a non-zero input": lambda w, xq: _head64(w, _fc1_64(w, _stop_at_thread_last(xq))),
    "LayerNorm with unbiased variance": lambda w, xq: _head64(w, _fc1_64(w, xq), _ln_unbiased, _ln_unbiased),
    "eps outside the square root": lambda w, xq: _head64(w, _fc1_64(w, xq), _ln_eps_outside, _ln_eps_outside),
    "one-pass variance in f32": lambda w, xq: _head64(w, _fc1_64(w, xq), _ln_one_pass_f32),
    "the c1 row of the neighbouring source": lambda w, xq: _head64(w, _fc1_64(w, xq, c1=np.roll(w.c1, -1, axis=0))),
    "the embedding of model 0 for every source": lambda w, xq: _head64(w, _fc1_64(w, xq, model_of_source=np.zeros(w.n_sources, np.int64))),
}


def mask_ignoring_threshold(w, logits):
    return np.asarray(logits) > 0


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, w, xq, **meta):
        self.name, self.w, self.xq, self.meta = name, w, np.ascontiguousarray(xq, dtype=np.float32), meta
        self.nq = self.xq.shape[0]
        assert self.xq.shape[1:] == (w.n_models, w.d_max)
        assert_exact_fc1(w, self.xq)

    @functools.cached_property
    def ref(self):
        return folded_forward64(self.w, self.xq)[0]

    @functools.cached_property
    def e32(self):
        """Largest deviation of the three f32 restatements from the float64 reference over the case's rows."""
        return float(max(np.abs(forward32(self.w, self.xq, o).astype(np.float64) - self.ref).max() for o in ORDERS))

    @property
    def tol(self):
        return MARGIN * self.e32


def column_queries(d_max, seed):
    """One one-hot row e_k per column k, model 1 seeing e_(d_max-1-k); one all-zero row; 37 dense integer rows.  Both load paths of
    router_fc1_kernel and its partial last chunk by the widths, every quarter boundary of the small kernel (kend = k + 1 for every
    k), 64-query tiles with one live chunk."""
    x = np.zeros((d_max + 38, 2, d_max), np.float32)
    k = np.arange(d_max)
    x[k, 0, k] = 1
    x[k, 1, d_max - 1 - k] = 1
    x[d_max + 1:] = int_queries(np.random.default_rng(seed), 37, 2, d_max)
    return x


def tile_queries(seed, d_max=130):
    """Three 64-query tiles: dense; model 0 all zero (a tile with NO live chunk) beside a dense model 1; and a tile whose queries have
    different live chunks (even rows only columns below 128, odd rows only the columns from 128 on) beside an all-zero model 1."""
    x = int_queries(np.random.default_rng(seed), 192, 2, d_max)
    x[64:128, 0] = 0
    x[128:192, 1] = 0
    x[128:192:2, 0, 128:] = 0
    x[129:192:2, 0, :128] = 0
    return x


def tail_queries(seed, d_max=770, nq=70):
    """Embeddings zero from column p on, p cycling through TAIL_STARTS (model 1 three steps ahead) with a full-width row every 7th:
    mixed inside every group of 4 and inside the 64-query tile."""
    x = int_queries(np.random.default_rng(seed), nq, 2, d_max)
    x[x == 0] = 1                                    # the last column before p is non-zero: p IS where the zeros begin
    starts = np.full((nq, 2), d_max)
    for q in range(nq):
        if q % 7 != 6:
            starts[q] = TAIL_STARTS[q % 6], TAIL_STARTS[(q + 3) % 6]
            x[q, 0, starts[q, 0]:] = 0
            x[q, 1, starts[q, 1]:] = 0
    return x, starts


def small_variance_queries(d_max=130, nq=40):
    """16 all-zero queries (fc1 = c1[c]: variance about 24 x 2^-18, near eps), 8 zero for model 0 and one-hot for model 1, 16 one-hot."""
    x = np.zeros((nq, 2, d_max), np.float32)
    for q in range(16, nq):
        x[q, 1, (7 * q) % d_max] = 1
        if q >= 24:
            x[q, 0, (11 * q) % d_max] = 2
    return x


def max_width_queries(nq=33):
    x = np.zeros((nq, 1, MAX_DMAX), np.float32)
    x[0::2, 0, MAX_DMAX - 1] = 1      # query 0 (the one a single-query call sends) is one-hot at the LAST column
    x[1::2, 0, 0] = 2
    return x


TOPOLOGIES = {   # name: (model_of_source, n_models, matrix-core form at 70 queries)
    "1x1": ((0,), 1, False),
    "5x1": ((0,) * 5, 1, False),                     # n_models == 1 and fewer than 8 sources: the small kernel at any batch size
    "8x1": ((0,) * 8, 1, True),
    "9-on-model-0-of-2": ((0,) * 9, 2, True),        # model 1 has no source
    "33x3-interleaved": (tuple(2 * (c % 2) for c in range(33)), 3, True),    # unsorted, model 1 unused, 17 sources on model 0
}


def _with_mask_bias(case, thr):
    """b3 that puts the median logit on the decision boundary log(thr / (1 - thr)): logits fall on both sides."""
    ref0 = folded_forward64(case.w.replace(b3=0.0), case.xq)[0]
    t = np.float64(np.float32(thr))
    return Case(case.name, case.w.replace(b3=np.float32(np.log(t / (1 - t)) - np.median(ref0)), thr=thr), case.xq)


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.partition(":")
    rng = np.random.default_rng(sum(name.encode()) + 1000 * len(name))
    if kind == "columns":
        d = int(arg)
        return Case(name, exact_weights(100 + d, d, DEFAULT_TOPOLOGY), column_queries(d, d))
    if kind == "tiles":
        return Case(name, exact_weights(7, 130, DEFAULT_TOPOLOGY), tile_queries(8))
    if kind == "ragged":
        return Case(name, exact_weights(9, 130, RAGGED_TOPOLOGY), int_queries(rng, max(RAGGED_NQ), 8, 130))
    if kind == "topology":
        mos, n_models, _ = TOPOLOGIES[arg]
        return Case(name, exact_weights(11 + len(mos), 130, mos, n_models), int_queries(rng, 70, n_models, 130))
    if kind == "layernorm":
        if arg == "small-variance":
            return Case(name, exact_weights(21, 130, DEFAULT_TOPOLOGY, c1_exp=-9), small_variance_queries())
        if arg == "mean-4096":
            x = int_queries(rng, 40, 2, 130)
            x[:16] = 0                                # fc1 = 4096 + integers in [-8, 8]: variance 24 on a mean of 4096
            return Case(name, exact_weights(22, 130, DEFAULT_TOPOLOGY, c1_offset=4096), x)
        if arg == "constant-row":
            return Case(name, exact_weights(23, 130, DEFAULT_TOPOLOGY, zero_w1q=True, constant_c1=True), int_queries(rng, 40, 2, 130))
    if kind == "tails":
        x, starts = tail_queries(31)
        return Case(name, exact_weights(32, 770, DEFAULT_TOPOLOGY), x, starts=starts)
    if kind == "nan-base":
        x = int_queries(rng, 70, 2, 130)
        g0 = NAN_QUERY - NAN_QUERY % 4
        x[NAN_QUERY, 0] = 0                           # the NaN will be this query's only non-zero input of model 0 ...
        x[g0:g0 + 4, 0, 100:] = 0                     # ... and, in the last column, past every input of its three group neighbours
        return Case(name, exact_weights(41, 130, DEFAULT_TOPOLOGY), x)
    if kind == "mask":
        return _with_mask_bias(Case(name, exact_weights(51, 130, DEFAULT_TOPOLOGY), int_queries(rng, 40, 2, 130)), float(arg))
    if kind == "max-width":
        return Case(name, exact_weights(61, MAX_DMAX, (0,) * 8), max_width_queries())
    raise KeyError(name)


NAN_QUERY = 5                    # group neighbours 4, 6, 7; tile neighbours 0 ... 63
NAN_COLUMNS = (3, 129)           # below 128, and the last column (the partial chunk; alone it decides where the k loop ends)
CASE_NAMES = ([f"columns:{d}" for d in COLUMN_WIDTHS] + ["tiles", "ragged"] + [f"topology:{t}" for t in TOPOLOGIES]
              + ["layernorm:small-variance", "layernorm:mean-4096", "layernorm:constant-row", "tails", "nan-base", "mask:0.4924", "mask:0.5",
                 "max-width"])


def with_nan(base, column):
    x = base.xq.copy()
    x[NAN_QUERY, 0, column] = np.nan
    return x


# ---- which rows catch which wrong kernel (tests/test_router_refs.py) ----------------------------------------------------------------------
def rows_on_model(w, m):
    return np.flatnonzero(w.model_of_source == m)


def catchers():
    """(stand-in name, case name, (query rows, source columns)) - the rows of the case that are meant to catch the stand-in."""
    m0, m1 = rows_on_model(case("columns:130").w, 0), rows_on_model(case("columns:130").w, 1)
    allc = np.arange(9)
    out = []
    for d in COLUMN_WIDTHS:
        out.append(("fc1 drops the last column", f"columns:{d}", ([d - 1], m0)))       # e_(d-1) for model 0
        out.append(("fc1 drops the last column", f"columns:{d}", ([0], m1)))           # model 1 sees e_(d-1) in query 0
    for d in (100, 130, 132, 770):       # widths with columns past a multiple of 128
        lo = d // 128 * 128
        out.append(("fc1 drops the columns past the last multiple of 128", f"columns:{d}", (list(range(lo, d)), m0)))
    for d in (1, 130, 770):              # widths that are no multiple of 4
        lo = d // 4 * 4
        out.append(("fc1 drops the columns past the last multiple of 4", f"columns:{d}", (list(range(lo, d)), m0)))
    # groups of 4 one-hot rows e_4g ... e_4g+3: query 0 of the group ends first, its three neighbours lose their only input
    out.append(("fc1 stops at the last non-zero input of query 0 of a group", "columns:130", ([1, 2, 3, 65, 66, 67, 125, 126, 127], m0)))
    starts = case("tails").meta["starts"]
    longer = [q for q in range(70) if starts[q, 0] > starts[q - q % 4, 0]]
    out.append(("fc1 stops at the last non-zero input of query 0 of a group", "tails", (longer, m0)))
    # found by the 770-wide column case on the GPU (deviation 0.279, the figure this stand-in gives): the row one-hot at the last
    # column and dense rows lost their last columns where the thread that saw them went on to a non-zero input of a later query
    for name in ("columns:770", "tails"):
        x = case(name).xq
        cut = _stop_at_thread_last(x)
        for m, cols in ((0, m0), (1, m1)):
            lost = np.flatnonzero((cut[:, m] != x[:, m]).any(1))
            if name == "columns:770" and m == 0:
                assert 769 in lost and lost.size >= 2, "the one-hot row of the last column and dense rows expose the defect"
            if lost.size:
                out.append(("fc1 stops where a thread last saw a non-zero input", name, (lost.tolist(), cols)))
    out.append(("LayerNorm with unbiased variance", "ragged", (list(range(129)), np.arange(13))))
    out.append(("eps outside the square root", "layernorm:small-variance", (list(range(16)), allc)))     # the all-zero queries
    out.append(("eps outside the square root", "layernorm:small-variance", (list(range(16, 24)), m0)))
    out.append(("one-pass variance in f32", "layernorm:mean-4096", (list(range(16)), allc)))
    out.append(("the c1 row of the neighbouring source", "topology:33x3-interleaved", (list(range(70)), np.arange(33))))
    out.append(("the c1 row of the neighbouring source", "columns:130", (list(range(168)), allc)))
    out.append(("the embedding of model 0 for every source", "columns:130", (list(range(130)), m1)))
    out.append(("the embedding of model 0 for every source", "ragged", (list(range(129)), np.flatnonzero(np.array(RAGGED_TOPOLOGY) != 0))))
    return out
