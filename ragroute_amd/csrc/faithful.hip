// f32-faithful exact search (rr_flat_search_faithful / rr_flat_search_f32_exact).
//
// The corpus keeps its f32 rows x beside the f16/bf16 copy x~ the scan kernels stream.  A search runs the ordinary segmented
// scan on the half copy with k' = list_len, re-scores the listed rows from the f32 rows (f64 accumulation, f32 rounding: the
// scores FAISS's IndexFlatIP would compute from the same f32 inputs, up to its own summation order) and proves the result:
//     s(x) = q.x = q~.x~ + (q - q~).x + q~.(x - x~)   and   |fl(q~.x~) - q~.x~| <= gamma(dim) |q~| |x~|
//  => s(x) <= s~(x) + eps(q),   eps(q) = c (|q - q~| Xmax + |q~| Dmax) + gamma(dim) |q~| X~max
// every row outside the list has a scan score s~(x) <= s~_L (the list's last), hence a true score <= s~_L + eps; if that,
// rounded up to f32, is strictly below the k-th re-scored f32 score, the k best re-scored rows are the exact top-k of the f32
// corpus, ties included (d_exact[q] = 1).  Queries whose proof fails are repeated with a longer list by the caller and, last,
// answered by faithful_scan_kernel: a plain brute-force f32 scan.
//
// Every f32 score of this file is the f32 rounding of an f64 sum over the elements in ascending order, one thread per (row,
// query): f64 addition is not associative, and this is the order of a plain sequential CPU scan, the
// checker the results are bit-compared with.  The
// f32 x f32 products are exact in f64, so fma and multiply-then-add give the same sums.
// No reference counterpart: the reference's faiss.IndexFlatIP scans every f32 row (data_source.py:158,186,203).
//
// Squared L2 (rr_flat_search_faithful_l2 / rr_flat_search_f32_exact_l2; the metric is a template argument of the re-score, scan
// and emit kernels).  D(q, x) = f32 rounding of acc_d, acc_{j+1} = fma(t_j, t_j, acc_j), t_j = (double)q_j - (double)x_j, j
// ascending: here the fma IS part of the definition (t_j is exact, t_j^2 is not).  Rows by D ascending, ties by ascending row,
// zero as +0.0, NaN never returned, a distance that rounds to +inf is a real row behind the finite ones, padding (+inf, -1).
// Rows are keyed by -D, so the descending sorts and merges list the nearest first.  The proof, with a = q~, b = x~:
//     the L2 scan ranks by s~ = fl(fl(a.b) - h(b)), h = fl(|b|^2 / 2) (rr_half_sqnorms); in every kernel the norm is taken off
//     the finished dot product by one f32 subtraction (the wide-row kernels ahead of the epilogue, the row-split kernel after
//     its halves are summed), and finalize_kernel<.., L2> reports D~ = fl(qn - 2 s~), qn = fl(|a|^2);
//     exactly |a - b|^2 = |a|^2 - 2 (a.b - |b|^2 / 2), and with X = X~max >= |b|, g = gamma(dim), u = one f32 rounding:
//       |fl(a.b) - a.b| <= g |a| X,  |h - |b|^2/2| <= g X^2 / 2,  |qn - |a|^2| <= g |a|^2,
//       the subtraction errs by <= u (|a| X + X^2/2)(1 + g), the finalize by <= u/(1-u) |D~|, |D~| <= (|a| + X)^2 (1 + g)(1 + u)
//  => |a - b|^2 >= D~ - A(q),  A(q) = g (2 |a| X + X^2 + |a|^2) + 4 2^-23 (|a| + X)^2 + 4 dim 2^-120 (1 + |a| + X)
//     (the u terms sum to < 2 u (|a| + X)^2 (1 + g)(1 + u) with u = 2^-24: A carries 8x that; the last term is the bf16
//     flush-to-zero term of eps(q) for the dot product, both norms and a subnormal difference)
// every row outside a list of length L has s~ <= s~_L, hence D~ >= D~_L (D~ is non-increasing in s~) and
//     |q - x| >= |a - b| - |q - q~| - |x - x~| >= sqrt(max(0, D~_L - A(q))) - R(q),   R(q) = |q - q~| + Dmax
// d_exact[q] = 1 when A and R are finite and the list's last entry is padding, or sqrt(max(0, D~_L - A)) > R and
// (sqrt(max(0, D~_L - A)) - R)^2, rounded DOWN to f32, is STRICTLY greater than the k-th re-scored distance: f32 rounding is
// monotone, so no outside row can reach or tie it.  A is +inf where |a| X, X^2 or |a|^2 nears f32's range, NaN where an input
// is not finite; neither certifies.  Dmax and X~max are stats words [0] and [2]: faithful_stats_kernel serves both metrics.
// (DESIGN.md "f32-faithful mode" has the derivation line by line.)
#include "rr_common.h"
#include "rr_kernels.h"
#include "rr_sort.h"

namespace rr {

namespace {

__device__ __forceinline__ double wsum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// smallest f32 >= v (NaN stays NaN)
__device__ __forceinline__ float up_f32(double v) {
  float f = (float)v;
  if ((double)f < v) {
    const uint32_t b = __float_as_uint(f);
    if ((b & 0x7FFFFFFFu) == 0) f = __uint_as_float(1u);
    else f = __uint_as_float((b & 0x80000000u) ? b - 1 : b + 1);
  }
  return f;
}

// largest f32 <= v (NaN stays NaN)
__device__ __forceinline__ float down_f32(double v) {
  float f = (float)v;
  if ((double)f > v) {
    const uint32_t b = __float_as_uint(f);
    if ((b & 0x7FFFFFFFu) == 0) f = __uint_as_float(0x80000001u);
    else f = __uint_as_float((b & 0x80000000u) ? b + 1 : b - 1);
  }
  return f;
}

// order key of a re-scored row: -0 and +0 are one score (scores compare with ==), NaN scores are never returned
__device__ __forceinline__ uint64_t score_key(float s, uint32_t row) {
  if (s != s) return 0ull;
  return make_key(s == 0.f ? 0.f : s, row);
}

// L2: a row is keyed by -D, so that the descending sorts and merges of this file list the nearest row first and equal distances
// by ascending row; the distance comes back out of a key's score as +0.0 for zero (never -0.0), +inf for a row that far away
__device__ __forceinline__ float dist_of_score(float s) { return s == 0.f ? 0.f : -s; }

__device__ __forceinline__ int seg_of(const FaithSegs& g, uint32_t row) {
  for (uint32_t s = 0; s < g.n; ++s)
    if (row >= g.row_begin[s] && row < g.row_limit[s]) return (int)s;
  return -1;  // alignment gap
}

// f64 dot product of one f32 row with an f32 query in LDS, elements in ascending order
__device__ __forceinline__ double dot_f64(const float* __restrict__ x, const float* q, int d, bool vec4) {
  double acc = 0.0;
  if (vec4) {
    const float4* x4 = (const float4*)x;
    for (int j = 0; j < d / 4; ++j) {
      const float4 v = x4[j];
      acc = fma((double)v.x, (double)q[4 * j], acc);
      acc = fma((double)v.y, (double)q[4 * j + 1], acc);
      acc = fma((double)v.z, (double)q[4 * j + 2], acc);
      acc = fma((double)v.w, (double)q[4 * j + 3], acc);
    }
  } else {
    for (int j = 0; j < d; ++j) acc = fma((double)x[j], (double)q[j], acc);
  }
  return acc;
}

// f64 squared distance of one f32 row from an f32 query in LDS: acc = fma(t, t, acc), t = (double)q_j - (double)x_j (exact), j
// ascending.  The fma is written out: t * t is NOT exact in f64, so multiply-then-add would round twice and give other sums.
__device__ __forceinline__ double sqdist_f64(const float* __restrict__ x, const float* q, int d, bool vec4) {
  double acc = 0.0;
  if (vec4) {
    const float4* x4 = (const float4*)x;
    for (int j = 0; j < d / 4; ++j) {
      const float4 v = x4[j];
      const double t0 = (double)q[4 * j] - (double)v.x, t1 = (double)q[4 * j + 1] - (double)v.y;
      const double t2 = (double)q[4 * j + 2] - (double)v.z, t3 = (double)q[4 * j + 3] - (double)v.w;
      acc = fma(t0, t0, acc);
      acc = fma(t1, t1, acc);
      acc = fma(t2, t2, acc);
      acc = fma(t3, t3, acc);
    }
  } else {
    for (int j = 0; j < d; ++j) {
      const double t = (double)q[j] - (double)x[j];
      acc = fma(t, t, acc);
    }
  }
  return acc;
}

// the f32 score one (row, query) pair is ordered by: q.x, or -D(q, x) under the L2 metric
template <bool L2>
__device__ __forceinline__ float pair_score(const float* __restrict__ x, const float* q, int d, bool vec4) {
  if constexpr (L2) return -(float)sqdist_f64(x, q, d, vec4);
  else return (float)dot_f64(x, q, d, vec4);
}

// stats words (f32 bit patterns of non-negative values, so that an unsigned max is a float max; NaN sorts above +inf):
// [0] Dmax = max |x - x~|, [1] Xmax = max |x|, [2] X~max = max |x~|.  One wave per row.  A row whose f32 values hold a NaN
// scores NaN against every query and is never returned, so it is left out; a row that overflows the half type makes
// Dmax infinite and no query is proven (all go to the exact scan).
template <typename T>
__global__ __launch_bounds__(256) void faithful_stats_kernel(const float* __restrict__ xf, int64_t ld, const T* __restrict__ xb, int64_t n,
                                                             int d, int dim, uint32_t* stats) {
  const int lane = threadIdx.x & 63;
  const int64_t wpb = blockDim.x >> 6;
  uint32_t m0 = 0, m1 = 0, m2 = 0;
  for (int64_t row = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * wpb) {
    double e2 = 0.0, n2 = 0.0, h2 = 0.0;
    for (int j = lane; j < d; j += 64) {
      const double x = (double)xf[row * ld + j], h = (double)(float)xb[row * dim + j];
      e2 = fma(x - h, x - h, e2);
      n2 = fma(x, x, n2);
      h2 = fma(h, h, h2);
    }
    e2 = wsum_d(e2);
    n2 = wsum_d(n2);
    h2 = wsum_d(h2);
    if (n2 != n2) continue;
    m0 = max(m0, __float_as_uint(up_f32(sqrt(e2))) & 0x7FFFFFFFu);
    m1 = max(m1, __float_as_uint(up_f32(sqrt(n2))) & 0x7FFFFFFFu);
    m2 = max(m2, __float_as_uint(up_f32(sqrt(h2))) & 0x7FFFFFFFu);
  }
  if (lane == 0) {
    atomicMax(&stats[0], m0);
    atomicMax(&stats[1], m1);
    atomicMax(&stats[2], m2);
  }
}

// one wave: e2 = |q - q~|^2 and h2 = |q~|^2 of one query and its half copy (f64, in every lane)
template <typename T>
__device__ __forceinline__ void query_norms(const float* __restrict__ xq, const T* __restrict__ xqh, int d, int lane, double& e2, double& h2) {
  e2 = h2 = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double x = (double)xq[j], h = (double)(float)xqh[j];
    e2 = fma(x - h, x - h, e2);
    h2 = fma(h, h, h2);
  }
  e2 = wsum_d(e2);
  h2 = wsum_d(h2);
}

// one wave per query: eps(q) (module header), rounded up; +inf where the scan could overflow (|q~| X~max near FLT_MAX), NaN
// where an input is not finite — neither ever proves a list
template <typename T>
__global__ __launch_bounds__(256) void faithful_queries_kernel(const float* __restrict__ xq, const T* __restrict__ xqh, int nq, int d, int dim,
                                                               const uint32_t* __restrict__ stats, double gamma, float* __restrict__ eps) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (q >= nq) return;
  double e2, h2;
  query_norms(xq + (size_t)q * d, xqh + (size_t)q * dim, d, lane, e2, h2);
  if (lane == 0) {
    const double dmax = __uint_as_float(stats[0]), xmax = __uint_as_float(stats[1]), hmax = __uint_as_float(stats[2]);
    const double en = sqrt(e2), hn = sqrt(h2);
    // 1.0001: the f64 roundings of the norms above (relative 1e-16 each); the last term: products of bf16 values that leave
    // the f32 normal range (flushed to zero by the matrix cores), at most 2^-126 each.  Subnormal fp16 INPUTS need no term: the
    // matrix cores of gfx950 take them unflushed (measured: tests/test_wide_values_gpu.py::test_fp16_subnormal_rows_score_exactly is
    // bit-exact on rows of subnormals, and tests/test_exact_f32_gpu.py's subnormal cases of test_eps_bounds_the_half_precision_scan
    // hold with this bound), and an fp16 x fp16 product is at least 2^-48, far inside the f32 normal range
    double v = 1.0001 * (en * xmax + hn * dmax) + gamma * hn * hmax + (double)dim * 0x1p-120 * (1.0 + hn + hmax);
    if (hn * hmax > 1e37) v = __builtin_inf();
    eps[q] = up_f32(v);
  }
}

// one wave per query, L2 metric: bound[q] = (A(q), R(q)) of the module header, each rounded up.  A is +inf where |q~| X~max, X~max^2
// or |q~|^2 nears f32's range (the scan's f32 arithmetic could overflow), NaN where an input is not finite — neither certifies
template <typename T>
__global__ __launch_bounds__(256) void faithful_queries_l2_kernel(const float* __restrict__ xq, const T* __restrict__ xqh, int nq, int d, int dim,
                                                                  const uint32_t* __restrict__ stats, double gamma, float* __restrict__ bound) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (q >= nq) return;
  double e2, h2;
  query_norms(xq + (size_t)q * d, xqh + (size_t)q * dim, d, lane, e2, h2);
  if (lane == 0) {
    const double dmax = __uint_as_float(stats[0]), hmax = __uint_as_float(stats[2]);
    const double en = sqrt(e2), hn = sqrt(h2), u = 0x1p-23;
    // gamma terms: dot product (x2), row norm, query norm; 4 u (|a| + X~max)^2: the two single roundings (u = 2^-23 where round to
    // nearest gives 2^-24: 8x what the derivation needs); 1.0001: the f64 roundings of the norms above; last term: products that
    // leave the f32 normal range (bf16 only, at most 2^-126 each, in the dot product and both norms) and subnormal differences
    double a = 1.0001 * (gamma * (2.0 * hn * hmax + hmax * hmax + hn * hn) + 4.0 * u * (hn + hmax) * (hn + hmax)) +
               4.0 * (double)dim * 0x1p-120 * (1.0 + hn + hmax);
    if (hn * hmax > 1e37 || hmax * hmax > 1e37 || hn * hn > 1e37) a = __builtin_inf();
    bound[2 * (size_t)q] = up_f32(a);
    bound[2 * (size_t)q + 1] = up_f32(1.0001 * en + dmax);
  }
}

// one workgroup per query: f32 scores of the listed rows (matrix rows, one thread per row), sort by (score, row), emit the
// top k with ids mapped through the segment table, certify
template <bool L2>
__global__ __launch_bounds__(256) void faithful_rescore_kernel(const float* __restrict__ xf, int64_t ld, int d, const float* __restrict__ xq, int L,
                                                               const float* __restrict__ PL, const int64_t* __restrict__ IL,
                                                               const float* __restrict__ eps, int k, const FaithSegs segs,
                                                               const uint8_t* __restrict__ mask, int64_t mask_stride,
                                                               float* __restrict__ D, int64_t* __restrict__ I, uint8_t* __restrict__ exact) {
  __shared__ float qf[kMaxDim];
  __shared__ uint64_t keys[kMaxK];
  const uint32_t q = blockIdx.x;
  for (int i = threadIdx.x; i < d; i += blockDim.x) qf[i] = xq[(size_t)q * d + i];
  const int np = pow2_ceil(L < 2 ? 2 : L);
  for (int i = L + threadIdx.x; i < np; i += blockDim.x) keys[i] = 0;
  const bool vec4 = (d & 3) == 0 && (ld & 3) == 0 && (((uintptr_t)xf) & 15) == 0;
  __syncthreads();
  for (int c = threadIdx.x; c < L; c += blockDim.x) {
    const int64_t row = IL[(size_t)q * L + c];
    // only rows of a segment routed to q are scored (the list is the top list_len of a set that holds all of them, so a row
    // outside it still scores <= the list's last)
    const int s = row >= 0 ? seg_of(segs, (uint32_t)row) : -1;
    const bool routed = s >= 0 && (segs.mask_col[s] < 0 || !mask || mask[(size_t)q * mask_stride + segs.mask_col[s]]);
    keys[c] = routed ? score_key(pair_score<L2>(xf + row * ld, qf, d, vec4), (uint32_t)row) : 0ull;
  }
  __syncthreads();
  bitonic_sort_desc(keys, np);
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    const uint64_t key = keys[i];  // k <= L <= np
    int64_t id = -1;
    if (key) {
      const uint32_t row = key_id(key);
      const int s = seg_of(segs, row);
      id = s >= 0 ? segs.id_offset[s] + (int64_t)(row - segs.row_begin[s]) : -1;
    }
    if constexpr (L2) D[(size_t)q * k + i] = key ? dist_of_score(key_score(key)) : __builtin_inff();
    else D[(size_t)q * k + i] = key ? key_score(key) : -__builtin_inff();
    I[(size_t)q * k + i] = id;
  }
  if (threadIdx.x == 0) {
    // `finite`: no input overflowed the half type, no NaN - every row the scan could rank is in its order.  `beats`: the bound on
    // every row outside the list, rounded towards the k-th re-scored row, stays strictly on its far side
    const float tail = PL[(size_t)q * L + L - 1];
    const uint64_t kth = keys[k - 1];
    const bool have = kth != 0 && tail - tail == 0.f;
    bool finite, beats = false;
    if constexpr (L2) {  // eps = bound [nq][2] = (A, R); tail = D~_L, the largest distance the half-precision search reports
      const float A = eps[2 * (size_t)q], R = eps[2 * (size_t)q + 1];
      finite = A - A == 0.f && R - R == 0.f;
      if (have) {
        // every row outside the list: |q - x| >= sqrt(max(0, D~_L - A)) - R.  (1 - 2^-40) twice: the f64 roundings of the
        // difference, the root and the square, and the relative error d 2^-53 of the f64 chain that such a row's own D sums
        const double m = (double)tail - (double)A;
        const double r = sqrt(m > 0.0 ? m : 0.0) * (1.0 - 0x1p-40) - (double)R;
        beats = r > 0.0 && down_f32(r * r * (1.0 - 0x1p-40)) > dist_of_score(key_score(kth));
      }
    } else {
      const float e = eps[q];
      finite = e - e == 0.f;
      beats = have && up_f32((double)tail + (double)e) < key_score(kth);
    }
    // a list whose last entry is padding holds every row the scan ranked: the whole (routed) corpus
    exact[q] = finite && (IL[(size_t)q * L + L - 1] < 0 || beats) ? 1 : 0;
  }
}

// Exact fallback: brute-force f32 scan of a block of nqb <= kScanQueries queries.  Workgroup g scans rows [g rpw, (g+1) rpw);
// one thread per row computes its scores against every query of the block (queries in LDS).  Per query the workgroup keeps
// its k best keys sorted in keys[0, k) and collects the keys of a 256-row tile that beat the current k-th in keys[k, k + 256);
// a tile that produced any is merged by one bitonic sort.  Output [nqb][G][k] (score, matrix row), padding (-inf, -1).
constexpr int kScanQueries = 16;
template <bool L2>
__global__ __launch_bounds__(256) void faithful_scan_kernel(const float* __restrict__ xf, int64_t ld, int d, int64_t n_rows,
                                                            const float* __restrict__ xq, const int32_t* __restrict__ qidx, int q0, int nqb,
                                                            int k, int P, int64_t rpw, const FaithSegs segs, const uint8_t* __restrict__ mask,
                                                            int64_t mask_stride, float* __restrict__ outD, int64_t* __restrict__ outI) {
  extern __shared__ uint64_t smem[];
  uint64_t* keys = smem;                                   // [nqb][P]
  uint64_t* thr = keys + (size_t)nqb * P;                  // [kScanQueries]
  uint32_t* cnt = (uint32_t*)(thr + kScanQueries);         // [kScanQueries]
  uint32_t* sel = cnt + kScanQueries;                      // [kScanQueries]
  float* qs = (float*)(sel + kScanQueries);                // [nqb][d]
  const int tid = threadIdx.x;
  const int G = gridDim.x, g = blockIdx.x;
  for (int b = 0; b < nqb; ++b) {
    const int64_t qi = qidx ? qidx[q0 + b] : q0 + b;
    for (int j = tid; j < d; j += blockDim.x) qs[(size_t)b * d + j] = xq[qi * d + j];
    for (int j = tid; j < P; j += blockDim.x) keys[(size_t)b * P + j] = 0;
    if (tid == 0) {
      uint32_t bits = 0;
      for (uint32_t s = 0; s < segs.n; ++s)
        if (segs.mask_col[s] < 0 || !mask || mask[qi * mask_stride + segs.mask_col[s]]) bits |= 1u << s;
      sel[b] = bits;
      cnt[b] = 0;
      thr[b] = 0;
    }
  }
  const bool vec4 = (d & 3) == 0 && (ld & 3) == 0 && (((uintptr_t)xf) & 15) == 0;
  const int64_t r0 = (int64_t)g * rpw, r1 = r0 + rpw < n_rows ? r0 + rpw : n_rows;
  __syncthreads();
  for (int64_t base = r0; base < r1; base += blockDim.x) {
    const int64_t row = base + tid;
    const int s = row < r1 ? seg_of(segs, (uint32_t)row) : -1;
    if (s >= 0) {
      double acc[kScanQueries];
#pragma unroll
      for (int b = 0; b < kScanQueries; ++b) acc[b] = 0.0;
      const float* x = xf + row * ld;
      if (vec4) {
        for (int j = 0; j < d / 4; ++j) {
          const float4 v = ((const float4*)x)[j];
#pragma unroll
          for (int b = 0; b < kScanQueries; ++b) {
            if (b < nqb) {
              const float* qb = qs + (size_t)b * d + 4 * j;
              if constexpr (L2) {
                const double t0 = (double)qb[0] - (double)v.x, t1 = (double)qb[1] - (double)v.y;
                const double t2 = (double)qb[2] - (double)v.z, t3 = (double)qb[3] - (double)v.w;
                acc[b] = fma(t0, t0, acc[b]);
                acc[b] = fma(t1, t1, acc[b]);
                acc[b] = fma(t2, t2, acc[b]);
                acc[b] = fma(t3, t3, acc[b]);
              } else {
                acc[b] = fma((double)v.x, (double)qb[0], acc[b]);
                acc[b] = fma((double)v.y, (double)qb[1], acc[b]);
                acc[b] = fma((double)v.z, (double)qb[2], acc[b]);
                acc[b] = fma((double)v.w, (double)qb[3], acc[b]);
              }
            }
          }
        }
      } else {
        for (int j = 0; j < d; ++j) {
          const double v = (double)x[j];
#pragma unroll
          for (int b = 0; b < kScanQueries; ++b) {
            if (b < nqb) {
              if constexpr (L2) {
                const double t = (double)qs[(size_t)b * d + j] - v;
                acc[b] = fma(t, t, acc[b]);
              } else {
                acc[b] = fma(v, (double)qs[(size_t)b * d + j], acc[b]);
              }
            }
          }
        }
      }
#pragma unroll
      for (int b = 0; b < kScanQueries; ++b) {
        if (b < nqb && ((sel[b] >> s) & 1u)) {
          const uint64_t key = score_key(L2 ? -(float)acc[b] : (float)acc[b], (uint32_t)row);
          if (key > thr[b]) {
            const uint32_t slot = atomicAdd(&cnt[b], 1u);  // < 256: one candidate per thread and tile
            keys[(size_t)b * P + k + slot] = key;
          }
        }
      }
    }
    __syncthreads();
    for (int b = 0; b < nqb; ++b) {
      const int c = (int)cnt[b];  // workgroup-uniform
      if (c == 0) continue;
      uint64_t* kb = keys + (size_t)b * P;
      const int n2 = pow2_ceil(k + c);
      for (int j = k + c + tid; j < n2; j += blockDim.x) kb[j] = 0;
      __syncthreads();
      bitonic_sort_desc(kb, n2);
      if (tid == 0) {
        thr[b] = kb[k - 1];
        cnt[b] = 0;
      }
      __syncthreads();
    }
  }
  for (int b = 0; b < nqb; ++b) {
    for (int j = tid; j < k; j += blockDim.x) {
      const uint64_t key = keys[(size_t)b * P + j];
      const size_t o = ((size_t)b * G + g) * k + j;
      outD[o] = key ? key_score(key) : -__builtin_inff();
      outI[o] = key ? (int64_t)key_id(key) : -1;
    }
  }
}

// block b of the fallback: (score, matrix row) [nqb][k] -> the caller's D / I rows qidx[q0 + b], ids through the segment table
template <bool L2>
__global__ __launch_bounds__(256) void faithful_emit_kernel(const float* __restrict__ Din, const int64_t* __restrict__ Iin, const int32_t* __restrict__ qidx,
                                                            int q0, int k, const FaithSegs segs, float* __restrict__ D, int64_t* __restrict__ I) {
  const int b = blockIdx.x;
  const int64_t qi = qidx ? qidx[q0 + b] : q0 + b;
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    const int64_t row = Iin[(size_t)b * k + j];
    int64_t id = -1;
    if (row >= 0) {
      const int s = seg_of(segs, (uint32_t)row);
      id = s >= 0 ? segs.id_offset[s] + (row - (int64_t)segs.row_begin[s]) : -1;
    }
    if constexpr (L2) D[qi * k + j] = id >= 0 ? dist_of_score(Din[(size_t)b * k + j]) : __builtin_inff();
    else D[qi * k + j] = id >= 0 ? Din[(size_t)b * k + j] : -__builtin_inff();
    I[qi * k + j] = id;
  }
}

int rows_grid(int64_t n) {
  int64_t g = (n + 3) / 4;
  if (g > 8192) g = 8192;
  return g < 1 ? 1 : (int)g;
}

}  // namespace

// gamma(dim): bound on |fl(q~.x~) - q~.x~| / (|q~| |x~|) of every scan kernel (DESIGN.md "f32-faithful mode").  The matrix
// cores form f16 x f16 and bf16 x bf16 products exactly in f32; what rounds is the summation, a tree over the dim products
// whatever its shape (K steps of the MFMA chain, the row-split halves, the wave reductions), of height < dim.  Each addition
// errs by less than one f32 ulp (2^-23 relative, which also covers a truncating adder), so the standard bound
// gamma_n = n u / (1 - n u) with n = dim and u = 2^-23 holds for all of them.
double faithful_gamma(int dim) {
  const double nu = (double)dim * 0x1p-23;
  return nu / (1.0 - nu);
}

FaithPlan faithful_plan(int k, int d, int grid, int64_t n_rows) {
  FaithPlan p;
  p.P = pow2_ceil_host(k + 256);
  const size_t per_query = (size_t)p.P * 8 + (size_t)d * 4, fixed = (size_t)kScanQueries * 16;
  int nqb = (int)((kFaithScanLds - fixed) / per_query);
  p.nqb = nqb > kScanQueries ? kScanQueries : nqb;
  p.gs = kSelectCap / k;
  int64_t G = grid;
  const int64_t tiles = (n_rows + 255) / 256;
  if (n_rows >= 0 && G > tiles) G = tiles < 1 ? 1 : tiles;
  if (G > p.gs) {
    if (G > (int64_t)p.gs * p.gs) G = (int64_t)p.gs * p.gs;
    G = G / p.gs * p.gs;
  }
  p.G = (int)G;
  p.lds = (size_t)p.nqb * per_query + fixed;
  return p;
}

hipError_t launch_faithful_build(const float* xf, int64_t ld, const void* xb, int dtype, int64_t n, int d, int dim, uint32_t* stats,
                                 hipStream_t st) {
  hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(uint32_t), st);
  if (e != hipSuccess || n == 0) return e;
  if (dtype == RR_DTYPE_F16)
    hipLaunchKernelGGL(faithful_stats_kernel<_Float16>, dim3(rows_grid(n)), dim3(256), 0, st, xf, ld, (const _Float16*)xb, n, d, dim, stats);
  else if (dtype == RR_DTYPE_BF16)
    hipLaunchKernelGGL(faithful_stats_kernel<__bf16>, dim3(rows_grid(n)), dim3(256), 0, st, xf, ld, (const __bf16*)xb, n, d, dim, stats);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_faithful_queries(const float* xq, const void* xqh, int dtype, int nq, int d, int dim, const uint32_t* stats, float* eps,
                                   hipStream_t st) {
  if (nq == 0) return hipSuccess;
  const int g = (nq + 3) / 4;
  const double gamma = faithful_gamma(dim);
  if (dtype == RR_DTYPE_F16)
    hipLaunchKernelGGL(faithful_queries_kernel<_Float16>, dim3(g), dim3(256), 0, st, xq, (const _Float16*)xqh, nq, d, dim, stats, gamma, eps);
  else if (dtype == RR_DTYPE_BF16)
    hipLaunchKernelGGL(faithful_queries_kernel<__bf16>, dim3(g), dim3(256), 0, st, xq, (const __bf16*)xqh, nq, d, dim, stats, gamma, eps);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_faithful_queries_l2(const float* xq, const void* xqh, int dtype, int nq, int d, int dim, const uint32_t* stats, float* bound,
                                      hipStream_t st) {
  if (nq == 0) return hipSuccess;
  const int g = (nq + 3) / 4;
  const double gamma = faithful_gamma(dim);
  if (dtype == RR_DTYPE_F16)
    hipLaunchKernelGGL(faithful_queries_l2_kernel<_Float16>, dim3(g), dim3(256), 0, st, xq, (const _Float16*)xqh, nq, d, dim, stats, gamma, bound);
  else if (dtype == RR_DTYPE_BF16)
    hipLaunchKernelGGL(faithful_queries_l2_kernel<__bf16>, dim3(g), dim3(256), 0, st, xq, (const __bf16*)xqh, nq, d, dim, stats, gamma, bound);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_faithful_rescore(bool l2, const float* xf, int64_t ld, int d, const float* xq, int nq, int L, const float* PL,
                                   const int64_t* IL, const float* eps, int k, const FaithSegs& segs, const uint8_t* mask,
                                   int64_t mask_stride, float* D, int64_t* I, uint8_t* exact, hipStream_t st) {
  if (nq == 0) return hipSuccess;
  hipLaunchKernelGGL(l2 ? faithful_rescore_kernel<true> : faithful_rescore_kernel<false>, dim3(nq), dim3(256), 0, st, xf, ld, d, xq, L, PL,
                     IL, eps, k, segs, mask, mask_stride, D, I, exact);
  return hipGetLastError();
}

hipError_t launch_faithful_scan(bool l2, const FaithPlan& p, const float* xf, int64_t ld, int d, int64_t n_rows, const float* xq, const int32_t* qidx,
                                int q0, int nqb, int k, const FaithSegs& segs, const uint8_t* mask, int64_t mask_stride, float* outD,
                                int64_t* outI, hipStream_t st) {
  int64_t rpw = (n_rows + p.G - 1) / p.G;
  rpw = (rpw + 255) / 256 * 256;
  hipLaunchKernelGGL(l2 ? faithful_scan_kernel<true> : faithful_scan_kernel<false>, dim3(p.G), dim3(256), p.lds, st, xf, ld, d, n_rows, xq,
                     qidx, q0, nqb, k, p.P, rpw, segs, mask, mask_stride, outD, outI);
  return hipGetLastError();
}

hipError_t launch_faithful_emit(bool l2, const float* Din, const int64_t* Iin, const int32_t* qidx, int q0, int nqb, int k, const FaithSegs& segs,
                                float* D, int64_t* I, hipStream_t st) {
  hipLaunchKernelGGL(l2 ? faithful_emit_kernel<true> : faithful_emit_kernel<false>, dim3(nqb), dim3(256), 0, st, Din, Iin, qidx, q0, k, segs,
                     D, I);
  return hipGetLastError();
}

}  // namespace rr
