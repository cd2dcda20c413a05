// Clustering a stored corpus (k-means): nearest-centroid assignment of every row, and the per-cluster means.
//  * cluster_assign_kernel : the scan's shape with another epilogue.  Rows stream from HBM once (A operand, straight into
//                            registers), the <= 64 centroids (B operand, L2 resident) are staged through LDS one K chunk at a
//                            time, mfma_f32_16x16x32 accumulates in f32, the epilogue subtracts the bias and takes the argmax
//                            over (score, lowest c) per row.
//  * cluster_sums_kernel   : each thread owns two columns and walks a fixed, argument-determined range of rows in order,
//                            adding into per-cluster f32 accumulators in LDS that it alone touches; at least every 4096 rows
//                            they are flushed into the range's own f64 partial in the workspace.  No float atomics.
//  * cluster_counts_kernel : members per (range, cluster), integer adds.
//  * cluster_means_kernel  : sums the per-range partials in range order (f64) and divides.
#include "rr_common.h"
#include "rr_kernels.h"

namespace rr {

// ---- assignment -------------------------------------------------------------------------------------------------------------
constexpr int kAsgTileRows = 128;     // rows per workgroup tile: 4 waves x 2 MFMA row tiles of 16
constexpr int kAsgChunk = 128;        // K elements per LDS stage (every padded dim is a multiple of 128)
constexpr int kAsgLdsStride = 144;    // halves per staged centroid row: 288 B = 72 dwords, so each 16-lane group of a ds_read_b128 (columns r, quarter h) hits 64 distinct banks

template <typename T> struct AsgMfma;
template <> struct AsgMfma<_Float16> {
  static __device__ __forceinline__ f32x4 run(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct AsgMfma<__bf16> {
  static __device__ __forceinline__ f32x4 run(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// One K chunk's operands as they come from memory: per lane its four 16-byte MFMA fragments of each of its two rows (A: step s of
// lane quarter h holds k = 32 s + 8 h ... + 8 of the chunk, so the four lanes of a row read 64 contiguous bytes per instruction)
// and its CT 16-byte pieces of the centroid chunk (B, on their way to LDS).
template <typename T, int CT>
struct AsgStage {
  typedef T vec8 __attribute__((ext_vector_type(8)));
  vec8 a[2][4];
  vec8 b[CT];
  __device__ __forceinline__ void load(const T* const (&pa)[2], const T* cent, int dim, int C, int k0, int tid) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int s = 0; s < 4; ++s) a[rt][s] = *(const vec8*)(pa[rt] + k0 + s * 32);
#pragma unroll
    for (int i = 0; i < CT; ++i) {
      const int p = i * 256 + tid, col = p >> 4, pc = p & 15;
      vec8 z;
#pragma unroll
      for (int e = 0; e < 8; ++e) z[e] = (T)0.f;
      b[i] = col < C ? *(const vec8*)(cent + (size_t)col * dim + k0 + pc * 8) : z;   // padding columns: zeros, masked in the epilogue
    }
  }
};

template <typename T, int CT>
__global__ __launch_bounds__(256) void cluster_assign_kernel(const T* __restrict__ xb, int64_t n_rows, int dim, const T* __restrict__ cent,
                                                             const float* __restrict__ bias, int C, int32_t* __restrict__ assign,
                                                             float* __restrict__ score, uint32_t n_tiles) {
  typedef T vec8 __attribute__((ext_vector_type(8)));
  __shared__ __attribute__((aligned(16))) T bs[CT * 16 * kAsgLdsStride];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, h = lane >> 4;
  float bv[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) bv[ct] = (bias && ct * 16 + r < C) ? bias[ct * 16 + r] : 0.f;

  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * kAsgTileRows + wave * 32;
    const T* pa[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      int64_t ra = row0 + rt * 16 + r;
      if (ra > n_rows - 1) ra = n_rows - 1;          // the last tile re-reads the last row: nothing at or beyond n_rows is touched
      pa[rt] = xb + ra * dim + h * 8;
    }
    f32x4 acc[2][CT];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    AsgStage<T, CT> next;
    next.load(pa, cent, dim, C, 0, tid);
    for (int k0 = 0; k0 < dim; k0 += kAsgChunk) {
      const AsgStage<T, CT> cur = next;
      __syncthreads();                               // the previous chunk's readers are done with bs
#pragma unroll
      for (int i = 0; i < CT; ++i) {
        const int p = i * 256 + tid;
        *(vec8*)(bs + (p >> 4) * kAsgLdsStride + (p & 15) * 8) = cur.b[i];
      }
      __syncthreads();
      if (k0 + kAsgChunk < dim) next.load(pa, cent, dim, C, k0 + kAsgChunk, tid);   // in flight under this chunk's MFMAs
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const vec8 b = *(const vec8*)(bs + (ct * 16 + r) * kAsgLdsStride + s * 32 + h * 8);
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) acc[rt][ct] = AsgMfma<T>::run(cur.a[rt][s], b, acc[rt][ct]);
        }
    }

    // C/D layout: col = lane & 15 (centroid ct * 16 + r), row = (lane >> 4) * 4 + reg.  Per row: the lane's best over its CT
    // columns (ascending c, strictly greater wins), then the best over the 16 lanes of the row's quarter.
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float best_s = 0.f;
        int best_c = -1;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const int c = ct * 16 + r;
          const float s = acc[rt][ct][reg] - bv[ct];
          if (c < C && s == s && (best_c < 0 || s > best_s)) { best_s = s; best_c = c; }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const float os = __shfl_xor(best_s, o, 64);
          const int oc = __shfl_xor(best_c, o, 64);
          if (oc >= 0 && (best_c < 0 || os > best_s || (os == best_s && oc < best_c))) { best_s = os; best_c = oc; }
        }
        const int64_t row = row0 + rt * 16 + h * 4 + reg;
        if (r == 0 && row < n_rows) {
          assign[row] = best_c;
          if (score) score[row] = best_c < 0 ? __builtin_nanf("") : best_s;
        }
      }
  }
}

template <typename T, int CT>
static hipError_t launch_assign_ct(const void* xb, int64_t n, int dim, const void* cent, const float* bias, int C, int32_t* assign,
                                   float* score, int cus, hipStream_t st) {
  const int64_t n_tiles = (n + kAsgTileRows - 1) / kAsgTileRows;       // n <= 2^32 - 32: fits 32 bits
  const int64_t resident = (CT == 1 ? 4ll : CT == 2 ? 3ll : 2ll) * cus;   // workgroups per CU by the registers of the instantiation
  const int64_t grid = n_tiles < resident ? n_tiles : resident;
  hipLaunchKernelGGL((cluster_assign_kernel<T, CT>), dim3((unsigned)grid), dim3(256), 0, st, (const T*)xb, n, dim, (const T*)cent, bias, C,
                     assign, score, (uint32_t)n_tiles);
  return hipGetLastError();
}

template <typename T>
static hipError_t launch_assign_t(const void* xb, int64_t n, int dim, const void* cent, const float* bias, int C, int32_t* assign,
                                  float* score, int cus, hipStream_t st) {
  switch ((C + 15) / 16) {
    case 1: return launch_assign_ct<T, 1>(xb, n, dim, cent, bias, C, assign, score, cus, st);
    case 2: return launch_assign_ct<T, 2>(xb, n, dim, cent, bias, C, assign, score, cus, st);
    case 3: return launch_assign_ct<T, 3>(xb, n, dim, cent, bias, C, assign, score, cus, st);
    case 4: return launch_assign_ct<T, 4>(xb, n, dim, cent, bias, C, assign, score, cus, st);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_cluster_assign(const void* xb, int dtype, int64_t n, int dim, const void* cent, const float* bias, int C,
                                 int32_t* assign, float* score, int cus, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (dtype == RR_DTYPE_F16) return launch_assign_t<_Float16>(xb, n, dim, cent, bias, C, assign, score, cus, st);
  if (dtype == RR_DTYPE_BF16) return launch_assign_t<__bf16>(xb, n, dim, cent, bias, C, assign, score, cus, st);
  return hipErrorInvalidValue;
}

// ---- means ------------------------------------------------------------------------------------------------------------------
constexpr int kMeansFlushRows = 4096;       // no f32 addition chain is longer than this
constexpr int kMeansBatch = 32;             // rows whose loads are in flight together (a multiple of 4)

// The plan depends on the arguments alone (never on the device), so the same arguments give the same additions in the same order.
ClusterMeansPlan cluster_means_plan(int64_t n, int dim, int C) {
  ClusterMeansPlan p;
  p.threads = C <= 32 ? 256 : 128;                                   // C x threads float2 accumulators: at most 64 KiB of LDS
  p.slabs = (dim + 2 * p.threads - 1) / (2 * p.threads);
  int64_t max_ranges = ((int64_t)1 << 27) / ((int64_t)C * dim * 8);  // about 128 MiB of f64 partials at the most
  if (max_ranges > 512) max_ranges = 512;
  if (max_ranges < 8) max_ranges = 8;
  int64_t ranges = (n + kMeansFlushRows - 1) / kMeansFlushRows;
  if (ranges > max_ranges) ranges = max_ranges;
  if (ranges < 1) ranges = 1;
  p.rows_per_range = (n + ranges - 1) / ranges;
  if (p.rows_per_range < 1) p.rows_per_range = 1;
  p.ranges = (int)((n + p.rows_per_range - 1) / p.rows_per_range);   // no empty range (n == 0: one, which writes zeros)
  if (p.ranges < 1) p.ranges = 1;
  p.sums_bytes = (size_t)p.ranges * C * dim * sizeof(double);
  p.total_bytes = p.sums_bytes + (size_t)p.ranges * C * sizeof(int64_t);
  return p;
}

template <typename T>
__global__ __launch_bounds__(256) void cluster_sums_kernel(const T* __restrict__ xb, int64_t n, int dim, const int32_t* __restrict__ assign, int C,
                                                           int64_t rows_per_range, double* __restrict__ sums) {
  typedef T vec2 __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) float2 acc[];   // [C][threads]; entry (c, t) belongs to thread t alone: no barrier anywhere
  const int t = threadIdx.x, T_ = blockDim.x;
  const int col = (blockIdx.y * T_ + t) * 2;
  if (col >= dim) return;                                        // the last slab's spare threads
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_range;
  const int64_t r1 = r0 + rows_per_range < n ? r0 + rows_per_range : n;
  for (int c = 0; c < C; ++c) acc[c * T_ + t] = float2{0.f, 0.f};
  double* my_sums = sums + (size_t)blockIdx.x * C * dim + col;
  bool first = true;
  int64_t rb = r0;
  do {
    const int64_t re = rb + kMeansFlushRows < r1 ? rb + kMeansFlushRows : r1;
    for (int64_t r = rb; r < re; r += kMeansBatch) {
      int32_t a[kMeansBatch];
      vec2 v[kMeansBatch];
#pragma unroll
      for (int i = 0; i < kMeansBatch; ++i) {                          // unconditional, so the batch's loads are in flight together:
        const int64_t ri = r + i < re ? r + i : re - 1;                // a row behind the block's end re-reads its last row
        a[i] = assign[ri];
        v[i] = *(const vec2*)(xb + ri * dim + col);
      }
#pragma unroll
      for (int i = 0; i < kMeansBatch; ++i)
        if (r + i >= re || (uint32_t)a[i] >= (uint32_t)C) a[i] = -1;   // -1 and anything else outside [0, C) is skipped
      // Rows are added strictly in order.  Four at a time: their accumulators are read together, a row whose cluster an earlier row
      // of the four already touched takes that row's sum instead of the stale read, and the sums are written back in order - the
      // additions and their order are those of the one-row-at-a-time loop, at a quarter of its LDS round trips.
#pragma unroll
      for (int g = 0; g < kMeansBatch; g += 4) {
        float2 s[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = a[g + i] >= 0 ? acc[a[g + i] * T_ + t] : float2{0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (a[g + i] < 0) continue;
#pragma unroll
          for (int j = 0; j < i; ++j)
            if (a[g + j] == a[g + i]) s[i] = s[j];                     // ascending j: the latest earlier row of this cluster wins
          s[i].x += (float)v[g + i][0];
          s[i].y += (float)v[g + i][1];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (a[g + i] >= 0) acc[a[g + i] * T_ + t] = s[i];
      }
    }
    for (int c = 0; c < C; ++c) {                                   // flush into this range's own f64 partial
      const float2 s = acc[c * T_ + t];
      double2 cur = first ? double2{0.0, 0.0} : *(const double2*)(my_sums + (size_t)c * dim);
      cur.x += (double)s.x;
      cur.y += (double)s.y;
      *(double2*)(my_sums + (size_t)c * dim) = cur;
      acc[c * T_ + t] = float2{0.f, 0.f};
    }
    first = false;
    rb = re;
  } while (rb < r1);
}

// Members per (range, cluster): integer adds, exact in any order.
__global__ __launch_bounds__(256) void cluster_counts_kernel(const int32_t* __restrict__ assign, int64_t n, int C, int64_t rows_per_range,
                                                             int64_t* __restrict__ counts) {
  __shared__ uint32_t cnt[RR_MAX_CLUSTERS];
  if (threadIdx.x < RR_MAX_CLUSTERS) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_range;
  const int64_t r1 = r0 + rows_per_range < n ? r0 + rows_per_range : n;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
    const int32_t a = assign[r];
    if ((uint32_t)a < (uint32_t)C) atomicAdd(&cnt[a], 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < C) counts[(size_t)blockIdx.x * C + threadIdx.x] = (int64_t)cnt[threadIdx.x];
}

__global__ __launch_bounds__(256) void cluster_means_kernel(const double* __restrict__ sums, const int64_t* __restrict__ counts, int ranges,
                                                            int C, int dim, int d, float* __restrict__ centroids,
                                                            int64_t* __restrict__ counts_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * d) return;
  const int c = i / d, j = i - c * d;
  int64_t m = 0;
  double s = 0.0;
  for (int g = 0; g < ranges; ++g) {                                // range order: fixed
    m += counts[(size_t)g * C + c];
    s += sums[((size_t)g * C + c) * dim + j];
  }
  if (m > 0) centroids[(size_t)c * d + j] = (float)(s / (double)m);  // a cluster without members keeps its row
  if (j == 0) counts_out[c] = m;
}

hipError_t launch_cluster_means(const void* xb, int dtype, int64_t n, int dim, int d, const int32_t* assign, int C, float* centroids,
                                int64_t* counts, void* ws, hipStream_t st) {
  const ClusterMeansPlan p = cluster_means_plan(n, dim, C);
  double* sums = (double*)ws;
  int64_t* part_counts = (int64_t*)((char*)ws + p.sums_bytes);
  const dim3 grid(p.ranges, p.slabs);
  const size_t lds = (size_t)C * p.threads * sizeof(float2);
  if (dtype == RR_DTYPE_F16)
    hipLaunchKernelGGL(cluster_sums_kernel<_Float16>, grid, dim3(p.threads), lds, st, (const _Float16*)xb, n, dim, assign, C, p.rows_per_range,
                       sums);
  else if (dtype == RR_DTYPE_BF16)
    hipLaunchKernelGGL(cluster_sums_kernel<__bf16>, grid, dim3(p.threads), lds, st, (const __bf16*)xb, n, dim, assign, C, p.rows_per_range,
                       sums);
  else
    return hipErrorInvalidValue;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cluster_counts_kernel, dim3(p.ranges), dim3(256), 0, st, assign, n, C, p.rows_per_range, part_counts);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cluster_means_kernel, dim3((C * d + 255) / 256), dim3(256), 0, st, sums, part_counts, p.ranges, C, dim, d, centroids,
                     counts);
  return hipGetLastError();
}

}  // namespace rr
