// C ABI of libragroute_hip.so (declared in include/ragroute_hip.h) and the host-side schedule of
// the flat search: bootstrap threshold -> geometrically growing scan chunks, each followed by an
// exact compaction that publishes the next per-query threshold -> finalize.  Everything is
// enqueued on the caller's stream; nothing here synchronises with the device.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>

#include "rr_common.h"
#include "rr_kernels.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* detail = "") {
  snprintf(g_err, sizeof(g_err), fmt, detail);
  return code;
}
int hip_status(hipError_t e, const char* where) {   // RR_OK, or RR_ERR_HIP with "where: what HIP says" recorded
  if (e == hipSuccess) return RR_OK;
  snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return RR_ERR_HIP;
}

int device_cus() {
  static thread_local int cached_dev = -1, cached = 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  if (dev != cached_dev) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    cached = v;
    cached_dev = dev;
  }
  return cached;
}

// ---- live profiling of the dominant kernel (bench.py roofline) -------------------------------------
struct ProfEntry { hipEvent_t start, stop; uint64_t rows; };
thread_local ProfEntry* g_prof = nullptr;
thread_local int g_prof_cap = 0, g_prof_n = 0, g_prof_dropped = 0;

hipError_t profiled_scan(const rr::ScanArgs& a, const rr::ScanPlan& plan, bool dense, int grid, hipStream_t st) {
  ProfEntry* p = g_prof && g_prof_n < g_prof_cap ? &g_prof[g_prof_n++] : nullptr;
  if (g_prof && !p) ++g_prof_dropped;   // rr_profile_end reports it: a silent drop would overstate the roofline
  if (p) { p->rows = (uint64_t)a.n_tiles * rr::kTileRows; (void)hipEventRecord(p->start, st); }
  const hipError_t e = rr::launch_flat_scan(a, plan, dense, grid, st);
  if (p) (void)hipEventRecord(p->stop, st);
  return e;
}

// Schedule knobs (defaults from rr_common.h; RR_SAMPLE_ROWS / RR_CHUNK_GROWTH override them for tuning runs)
int sample_rows() {
  static const int v = [] {
    const char* e = rr::tuning_env("RR_SAMPLE_ROWS");
    const int r = e ? atoi(e) / rr::kTileRows * rr::kTileRows : 0;
    return r >= 1024 && r <= rr::kSampleRows ? r : rr::kSampleRows;
  }();
  return v;
}
int chunk_growth() {   // 0 = the size-aware schedule
  static const int v = [] { const char* e = rr::tuning_env("RR_CHUNK_GROWTH"); const int g = e ? atoi(e) : 0; return g >= 2 && g <= 1024 ? g : 0; }();
  return v;
}

struct Bump {   // bump allocator of the workspace layouts: 256-byte aligned pieces; base == nullptr only measures
  char* base;
  size_t off = 0;
  template <typename T> T* take(size_t count) {
    const size_t o = off;
    off = (off + count * sizeof(T) + 255) / 256 * 256;
    return base ? (T*)(base + o) : nullptr;
  }
};

// Growth factor of the chunk schedule for a shard that is `ratio` times the bootstrap sample.  With c chunks the growth is
// g = ratio^(1/c) and every chunk leaves ~(g - 1) k survivors per query.  A workgroup sees every query, so it takes the
// insertion path ~(g - 1) k times per chunk, and its four waves wait for each other at the next tile barrier.  Cost model
// (MI355X, measured in round 2: a 2-chunk schedule at 10M rows ran 0.16 ms SLOWER than the 4-chunk one): ~37 us per chunk
// for the launch's fixed part and its compaction, ~0.18 us per insertion event of a workgroup.
// 1M x 768, k = 32 -> 3 chunks; 10M -> 4; 80M at k = 100 -> 6.
double chunk_schedule(double ratio, int k) {
  if (chunk_growth() > 0) return (double)chunk_growth();   // RR_CHUNK_GROWTH pins the round-1 schedule for A/B runs
  if (ratio <= 1.0) return 2.0;
  double best_cost = 1e30, best_g = 8.0;
  for (int c = 1; c <= 8; ++c) {
    const double g = pow(ratio, 1.0 / c);
    const double cost = c * (37.0 + 0.18 * (g - 1.0) * k);
    if (cost < best_cost) { best_cost = cost; best_g = g; }
  }
  return best_g < 1.5 ? 1.5 : best_g;
}

struct Workspace {
  uint32_t *seg_tile_end, *seg_row_limit, *seg_row_begin, *seg_sel;   // segmented search: device tables written by prep_kernel
  int64_t* seg_id_offset;
  rr::RangeEntry* ranges;                                             // [kMaxChunks][kMaxSegments] tile runs of the chunk launches
  float *thr, *dense;
  uint32_t *list_cnt, *cand_cnt;
  uint64_t *list, *scratch, *cand;
  void* xqs;
  size_t total;
};

Workspace carve(char* base, int k, int grid, int dtype, int dim) {
  using namespace rr;
  const size_t cap = cand_cap_for_k(k), nq = kQueriesPerBlock;
  const size_t nbuf = (size_t)grid * scan_max_bufs_per_wg(dtype, dim);   // candidate buffers per query of the widest plan at this dim
  Workspace w;
  Bump b{base};
  w.thr = b.take<float>(kMaxSegments * nq);   // [segment][query] (plain search: row 0)
  w.seg_tile_end = b.take<uint32_t>(kMaxSegments);
  w.seg_row_limit = b.take<uint32_t>(kMaxSegments);
  w.seg_row_begin = b.take<uint32_t>(kMaxSegments);
  w.seg_id_offset = b.take<int64_t>(kMaxSegments);
  w.seg_sel = b.take<uint32_t>(nq);
  w.ranges = b.take<RangeEntry>((size_t)kMaxChunks * kMaxSegments);
  w.list_cnt = b.take<uint32_t>(nq);
  w.list = b.take<uint64_t>(nq * kMaxK);
  w.cand_cnt = b.take<uint32_t>(nq * nbuf);
  w.scratch = b.take<uint64_t>((size_t)grid * 8 * cap);  // up to 2 workgroups per CU x 4 waves
  w.dense = b.take<float>(nq * kSampleRows);
  w.cand = b.take<uint64_t>(nq * nbuf * cap);
  w.xqs = b.take<char>(nq * kMaxDim * 2);  // the query block in MFMA-fragment order (prep kernel): 256 queries x the padded dim
  w.total = b.off;
  return w;
}

// ---- the schedule of one search ---------------------------------------------------------------------------------------------------
// One scan launch of the chunk schedule and the compaction behind it.  Plain search: tiles [tile_first, tile_first + n_tiles).
// Segmented: chunk `index` of the range tables prep_kernel writes, n_tiles launch ordinals in n_ranges runs; n_tiles == 0 (only the
// last chunk may be empty) compacts without a scan.
struct Chunk { uint32_t tile_first, n_tiles, index, n_ranges; };
// growth >= 1.5 from a sample of >= 32 tiles up to < 2^27 tiles: at most 38 chunks (product builds: chunk_schedule picks <= 8)
constexpr uint32_t kMaxPlainChunks = 40;
// The launches of a search as far as they depend on the corpus and the segments alone: computed once per call, run per query block.
struct Schedule { uint32_t total_tiles, n_sample_tiles, n_chunks; Chunk chunks[kMaxPlainChunks]; };

// Plain schedule: chunks [0,e1), [e1,e2), ... with e growing geometrically: a chunk that is g times what came before it yields
// ~(g-1) k survivors per query.  The number of chunks balances the fixed cost of a scan launch + compaction against the insertion
// work of a long chunk (chunk_schedule).
void plain_chunks(Schedule& sc, double growth) {
  uint64_t begin = 0;
  double endf = (double)sc.n_sample_tiles * growth;  // in tiles
  while (begin < sc.total_tiles) {
    uint64_t end = ((uint64_t)(endf + 0.5) + 7) & ~7ull;   // whole 256-row groups: the wide-row kernels' K order is a function of the global group (flat_scan_wide.hip)
    if (end > sc.total_tiles || (double)sc.total_tiles < endf * 1.25) end = sc.total_tiles;  // no sliver of a last chunk
    if (end <= begin) end = begin + 8;
    if (end > sc.total_tiles || sc.n_chunks + 1 == kMaxPlainChunks) end = sc.total_tiles;
    sc.chunks[sc.n_chunks++] = Chunk{(uint32_t)begin, (uint32_t)(end - begin), 0, 0};
    begin = end;
    endf *= growth;
  }
}

// Segmented schedule: chunk c takes the next slice of EVERY segment (seg_cut), reaching the cumulative fraction frac[c] of each, so
// that whatever subset of the segments a query is routed to, its rows arrive in geometrically growing portions.  frac[c] = sample
// share x growth^(c+1), the last one 1 (no sliver of a last chunk).  The launch sizes here and prep_kernel's range tables (from the
// same SegHost) use one expression.  A chunk that is empty in every segment is dropped, except the last: its compaction finalizes.
void segment_chunks(Schedule& sc, rr::SegHost& segs, double ratio, double growth) {
  using namespace rr;
  double f = growth / ratio;
  uint32_t nc = 0;
  for (; nc + 1 < (uint32_t)kMaxChunks && f * 1.25 < 1.0; ++nc, f *= growth) segs.frac[nc] = (uint32_t)(f * 4294967296.0);
  segs.frac[nc++] = 0xFFFFFFFFu;
  segs.n_chunks = nc;
  for (uint32_t c = 0; c < nc; ++c) {
    Chunk ch{0, 0, c, 0};
    for (uint32_t sg = 0; sg < segs.n; ++sg) {
      const uint32_t tiles = (segs.row_limit[sg] - segs.row_begin[sg] + kTileRows - 1) / kTileRows;
      const uint32_t lo = c ? seg_cut(tiles, segs.frac[c - 1]) : 0u, hi = seg_cut(tiles, segs.frac[c]);
      if (hi > lo) { ch.n_tiles += (hi - lo + 7u) & ~7u; ++ch.n_ranges; }
    }
    if (ch.n_tiles > 0 || c + 1 == nc) sc.chunks[sc.n_chunks++] = ch;
  }
}

// What the launches of one block of queries share.
struct Block { rr::ScanPlan plan; rr::SelectArgs s; rr::ScanArgs a; int grid; hipStream_t st; };

// All scores of n_tiles tiles, every tile_stride-th one of the corpus, and one exact selection from them.
int dense_pass(Block& b, uint32_t tile_stride, uint32_t n_tiles, bool bootstrap) {
  b.a.tile_first = 0; b.a.tile_stride = tile_stride; b.a.n_tiles = n_tiles;
  if (int rc = hip_status(profiled_scan(b.a, b.plan, true, b.grid, b.st), bootstrap ? "rr_flat_search/bootstrap" : "rr_flat_search/dense")) return rc;
  b.s.tile_first = 0; b.s.tile_stride = tile_stride; b.s.dense_cols = n_tiles * rr::kTileRows;
  return hip_status(rr::launch_dense_select(b.s, bootstrap, b.st), bootstrap ? "rr_flat_search/bootstrap_select" : "rr_flat_search/dense_select");
}
// tiny corpus: every row
int schedule_dense(Block& b, const Schedule& sc) { return dense_pass(b, 1, sc.total_tiles, false); }
// head of both chunk schedules: the k-th best score of a strided sample of tiles = a valid lower bound
int bootstrap(Block& b, const Schedule& sc) { return dense_pass(b, sc.total_tiles / sc.n_sample_tiles, sc.n_sample_tiles, true); }

// bootstrap, then scan + compaction per chunk.  fin != nullptr: the last compaction emits (D, I).
int schedule_chunks(Block& b, const Schedule& sc, const rr::FinalizeArgs* fin) {
  if (int rc = bootstrap(b, sc)) return rc;
  b.a.tile_stride = 1;
  b.a.timeline = rr::tuning_env("RR_SCAN_TIMELINE") ? (uint64_t*)b.a.dense : nullptr;  // the dense buffer is idle during chunk scans
  for (uint32_t i = 0; i < sc.n_chunks; ++i) {
    b.a.tile_first = sc.chunks[i].tile_first; b.a.n_tiles = sc.chunks[i].n_tiles;
    if (int rc = hip_status(profiled_scan(b.a, b.plan, false, b.grid, b.st), "rr_flat_search/scan")) return rc;
    if (int rc = hip_status(rr::launch_compact(b.s, i + 1 == sc.n_chunks ? fin : nullptr, b.st), "rr_flat_search/compact")) return rc;
  }
  return RR_OK;
}

// the same over the range tables (device [kMaxChunks][kMaxSegments], written by prep_kernel)
int schedule_segment_chunks(Block& b, const Schedule& sc, const rr::RangeEntry* ranges, const rr::FinalizeArgs* fin) {
  if (int rc = bootstrap(b, sc)) return rc;
  b.a.tile_first = 0; b.a.tile_stride = 1;
  for (uint32_t i = 0; i < sc.n_chunks; ++i) {
    const Chunk& c = sc.chunks[i];
    b.a.n_tiles = c.n_tiles; b.a.ranges = ranges + (size_t)c.index * rr::kMaxSegments; b.a.n_ranges = c.n_ranges;
    if (c.n_tiles > 0)
      if (int rc = hip_status(profiled_scan(b.a, b.plan, false, b.grid, b.st), "rr_flat_search_segments/scan")) return rc;
    if (int rc = hip_status(rr::launch_compact(b.s, i + 1 == sc.n_chunks ? fin : nullptr, b.st), "rr_flat_search_segments/compact")) return rc;
  }
  return RR_OK;
}

// What a search checks before it looks at a pointer (every entry point of the flat search reports these the same way).
int check_search_sizes(int dtype, int64_t n_rows, int dim, int nq, int k) {
  using namespace rr;
  if (k < 1 || k > kMaxK) return fail(RR_ERR_INVALID, "rr_flat_search: k must be in [1, 1024]%s");
  if (nq < 0 || n_rows < 0) return fail(RR_ERR_INVALID, "rr_flat_search: negative size%s");
  if (n_rows > 0xFFFFFFE0ll) return fail(RR_ERR_UNSUPPORTED, "rr_flat_search: more than 2^32-32 rows per shard%s");
  if (!half_dtype(dtype) && dtype != kDtypeI8) return fail(RR_ERR_INVALID, "rr_flat_search: bad dtype%s");
  if (scan_padded_dim(dim) != dim) return fail(RR_ERR_UNSUPPORTED, "rr_flat_search: dim must equal rr_padded_dim(d)%s");
  return RR_OK;
}

// segs != nullptr: segmented search — xb is ONE matrix of n_rows rows holding several sources (segs->row_begin / row_limit),
// scanned as one corpus; route_mask then is [nq][mask_stride] with one column per segment (segs->mask_col), id_offset unused.
// half_sqnorm != nullptr: the squared-L2 metric (|x|^2 / 2 per matrix row), plain or segmented: same schedules, the scan ranks by
// q.x - |x|^2/2 and launch_finalize turns the list into distances.
int flat_search_impl(const void* xb, int dtype, int64_t n_rows, int dim, const void* xq, int nq, int k, float* D, int64_t* I,
                     int64_t id_offset, void* ws, size_t ws_bytes, const uint8_t* route_mask, int64_t mask_stride,
                     const float* half_sqnorm, void* stream, rr::SegHost* segs = nullptr) {
  using namespace rr;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = check_search_sizes(dtype, n_rows, dim, nq, k)) return rc;
  if (nq == 0) return RR_OK;
  if (!xq || !D || !I || !ws || (!xb && n_rows > 0)) return fail(RR_ERR_INVALID, "rr_flat_search: null pointer%s");
  const int grid = device_cus();
  if (grid <= 0) return fail(RR_ERR_HIP, "rr_flat_search: no HIP device%s");
  const Workspace w = carve((char*)ws, k, grid, dtype, dim);
  if (ws_bytes < w.total) return fail(RR_ERR_WORKSPACE, "rr_flat_search: workspace smaller than rr_flat_search_workspace_bytes_for(k, dim)%s");

  const bool l2 = half_sqnorm != nullptr, chunked = n_rows > kDenseMaxRows;   // (up to kDenseMaxRows rows: the dense schedule)
  // THE decision on who writes (D, I): the last compaction of an inner-product chunk schedule does; every other search - L2, tiny or
  // empty corpus - ends with launch_finalize
  const bool compact_finalizes = chunked && !l2;
  Schedule sc{(uint32_t)((n_rows + kTileRows - 1) / kTileRows), (uint32_t)sample_rows() / kTileRows, 0, {}};
  if (chunked) {
    const double ratio = (double)sc.total_tiles / sc.n_sample_tiles, growth = chunk_schedule(ratio, k);
    if (segs) { segment_chunks(sc, *segs, ratio, growth); segs->ranges = w.ranges; }
    else plain_chunks(sc, growth);
  }

  const int cap = cand_cap_for_k(k);
  const int qpl = scan_queries_per_launch(dim, nq);  // 256, or 128 where only 32 queries per wave stay resident and the batch is small
  for (int qb = 0; qb < nq; qb += qpl) {
    const int nqb = nq - qb < qpl ? nq - qb : qpl;
    const char* xq_b = (const char*)xq + (size_t)qb * dim * 2;
    // (segmented: the per-query route mask rows of this query block are folded into the thresholds by prep, not into the finalize)
    const uint8_t* mask_b = route_mask ? route_mask + (size_t)qb * mask_stride : nullptr;
    const FinalizeArgs fin{D + (size_t)qb * k, I + (size_t)qb * k, id_offset, segs ? nullptr : mask_b, mask_stride};

    Block b;
    memset(&b, 0, sizeof(b));
    // (per query block: the kernel is picked from the block's own query count, e.g. the 44-query tail of a 300-query call)
    b.plan = scan_plan(dtype, dim, nqb, l2);
    b.grid = grid; b.st = st;
    SelectArgs& s = b.s;
    s.thr = w.thr; s.list = w.list; s.list_cnt = w.list_cnt; s.cand = w.cand; s.cand_cnt = w.cand_cnt;
    s.dense = w.dense; s.dense_ld = kSampleRows; s.n_rows = (uint32_t)n_rows; s.nq = (uint32_t)nqb;
    s.nbuf = (uint32_t)grid * (uint32_t)b.plan.bufs_per_wg; s.list_ld = kMaxK; s.cap = cap; s.k = k;
    if (segs) s.seg = SegTables{w.seg_tile_end, w.seg_row_limit, w.seg_row_begin, w.seg_id_offset, w.seg_sel, segs->n};
    ScanArgs& a = b.a;
    a.xb = xb; a.xq = xq_b; a.xqs = w.xqs; a.thr = w.thr; a.cand = w.cand; a.cand_cnt = w.cand_cnt; a.scratch = w.scratch;
    a.dense = w.dense; a.n_rows = (uint32_t)n_rows; a.nq = (uint32_t)nqb; a.dense_ld = kSampleRows; a.cap = cap; a.k = k;
    a.half_sqnorm = half_sqnorm;
    if (segs) a.ties_pass = 1;

    if (int rc = hip_status(launch_prep(s, xq_b, w.xqs, dim, b.plan.blocks_per_wave, st, segs, segs ? mask_b : nullptr, mask_stride),
                            "rr_flat_search/prep")) return rc;
    const FinalizeArgs* cfin = compact_finalizes ? &fin : nullptr;
    int rc = RR_OK;
    if (chunked) rc = segs ? schedule_segment_chunks(b, sc, w.ranges, cfin) : schedule_chunks(b, sc, cfin);
    else if (n_rows > 0) rc = schedule_dense(b, sc);
    if (rc != RR_OK) return rc;
    if (compact_finalizes) continue;
    if (int rc = hip_status(launch_finalize(s, fin.D, fin.I, fin.id_offset, fin.mask, fin.mask_stride, l2 ? (const void*)xq_b : nullptr,
                                            dtype, dim, st), "rr_flat_search/finalize")) return rc;
  }
  return RR_OK;
}

}  // namespace

// The compile flags of this library, written by ragroute_amd/_build.py next to the objects (its -I directory) before it compiles this unit.
#if __has_include("rr_build_flags.inc")
const char kBuildFlags[] =
#include "rr_build_flags.inc"
    ;
#else
const char kBuildFlags[] = "unknown (not built by ragroute_amd/_build.py)";
#endif

extern "C" {

int rr_version(void) { return 900; }  // 0.9.0: k-means over a stored corpus (rr_cluster_assign, rr_cluster_means, rr_cluster_workspace_bytes); 0.8.0: f32-faithful exact search under the squared-L2 metric (rr_flat_search_faithful_l2, rr_flat_search_f32_exact_l2); 0.7.0: segmented squared-L2 search (rr_flat_search_segments_l2); 0.6.0: f32-faithful exact search (rr_flat_search_faithful, rr_flat_search_f32_exact); 0.5.0: row-split wide-row kernel for L2 / any k / 193+ queries (8 candidate buffers per workgroup on wide rows at every k: larger workspace), tuning variables ignored by product builds, cursor-free plain scans
const char* rr_build_flags(void) { return kBuildFlags; }
const char* rr_last_error(void) { return g_err; }
int rr_device_cus(void) {
  int v = device_cus();
  return v > 0 ? v : fail(RR_ERR_HIP, "rr_device_cus: no HIP device%s");
}
int rr_padded_dim(int d) {
  if (d <= 0) return RR_ERR_INVALID;
  int p = rr::scan_padded_dim(d);
  return p > 0 ? p : RR_ERR_UNSUPPORTED;
}

int rr_l2_normalize_f32(float* x, int64_t n, int64_t d, void* stream) {
  if (n < 0 || d <= 0 || (!x && n > 0)) return fail(RR_ERR_INVALID, "rr_l2_normalize_f32: bad arguments%s");
  return hip_status(rr::launch_l2_normalize_f32(x, n, d, (hipStream_t)stream), "rr_l2_normalize_f32");
}

int rr_rows_to_half(const float* x, int64_t n, int64_t d, int64_t ld_in, void* out, int dtype, int64_t d_out,
                    int normalize, void* stream) {
  if (n < 0 || d <= 0 || ld_in < d || d_out < d || ((!x || !out) && n > 0))
    return fail(RR_ERR_INVALID, "rr_rows_to_half: bad arguments%s");
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_rows_to_half: bad dtype%s");
  return hip_status(rr::launch_rows_to_half(x, n, d, ld_in, out, dtype, d_out, normalize, (hipStream_t)stream), "rr_rows_to_half");
}

int rr_centroid(const void* xb, int dtype, int64_t n_rows, int dim, int d, float* out, void* stream) {
  if (n_rows < 0 || d < 1 || d > dim || dim % 64 != 0 || !out || (!xb && n_rows > 0))
    return fail(RR_ERR_INVALID, "rr_centroid: bad arguments%s");
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_centroid: bad dtype%s");
  return hip_status(rr::launch_centroid(xb, dtype, n_rows, dim, d, out, (hipStream_t)stream), "rr_centroid");
}

static bool cluster_sizes_ok(int64_t n_rows, int dim, int n_clusters) {
  return n_rows >= 0 && n_rows <= 0xFFFFFFE0ll && n_clusters >= 1 && n_clusters <= RR_MAX_CLUSTERS && dim > 0 && rr::scan_padded_dim(dim) == dim;
}

int rr_cluster_assign(const void* xb, int dtype, int64_t n_rows, int dim, const void* cent, const float* bias, int n_clusters,
                      int32_t* assign, float* score, void* stream) {
  if (n_rows < 0) return fail(RR_ERR_INVALID, "rr_cluster_assign: negative row count%s");
  if (n_clusters < 1 || n_clusters > RR_MAX_CLUSTERS) return fail(RR_ERR_INVALID, "rr_cluster_assign: n_clusters must be in [1, 64]%s");
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_cluster_assign: bad dtype%s");
  if (!cent || ((!xb || !assign) && n_rows > 0)) return fail(RR_ERR_INVALID, "rr_cluster_assign: null pointer%s");
  if (dim <= 0 || rr::scan_padded_dim(dim) != dim) return fail(RR_ERR_UNSUPPORTED, "rr_cluster_assign: dim must equal rr_padded_dim(d)%s");
  if (n_rows > 0xFFFFFFE0ll) return fail(RR_ERR_UNSUPPORTED, "rr_cluster_assign: more than 2^32-32 rows%s");
  if (n_rows == 0) return RR_OK;
  const int cus = device_cus();
  if (cus <= 0) return fail(RR_ERR_HIP, "rr_cluster_assign: no HIP device%s");
  return hip_status(rr::launch_cluster_assign(xb, dtype, n_rows, dim, cent, bias, n_clusters, assign, score, cus, (hipStream_t)stream),
                    "rr_cluster_assign");
}

size_t rr_cluster_workspace_bytes(int64_t n_rows, int dim, int n_clusters) {
  if (!cluster_sizes_ok(n_rows, dim, n_clusters)) return 0;
  return rr::cluster_means_plan(n_rows, dim, n_clusters).total_bytes;
}

int rr_cluster_means(const void* xb, int dtype, int64_t n_rows, int dim, int d, const int32_t* assign, int n_clusters, float* centroids,
                     int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (n_rows < 0) return fail(RR_ERR_INVALID, "rr_cluster_means: negative row count%s");
  if (n_clusters < 1 || n_clusters > RR_MAX_CLUSTERS) return fail(RR_ERR_INVALID, "rr_cluster_means: n_clusters must be in [1, 64]%s");
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_cluster_means: bad dtype%s");
  if (d < 1 || d > dim) return fail(RR_ERR_INVALID, "rr_cluster_means: d must be in [1, dim]%s");
  if (!centroids || !counts || !ws || ((!xb || !assign) && n_rows > 0)) return fail(RR_ERR_INVALID, "rr_cluster_means: null pointer%s");
  if ((uintptr_t)ws % 16 != 0) return fail(RR_ERR_INVALID, "rr_cluster_means: the workspace must be 16-byte aligned%s");
  if (rr::scan_padded_dim(dim) != dim) return fail(RR_ERR_UNSUPPORTED, "rr_cluster_means: dim must equal rr_padded_dim(d)%s");
  if (n_rows > 0xFFFFFFE0ll) return fail(RR_ERR_UNSUPPORTED, "rr_cluster_means: more than 2^32-32 rows%s");
  if (ws_bytes < rr::cluster_means_plan(n_rows, dim, n_clusters).total_bytes)
    return fail(RR_ERR_WORKSPACE, "rr_cluster_means: workspace smaller than rr_cluster_workspace_bytes%s");
  return hip_status(rr::launch_cluster_means(xb, dtype, n_rows, dim, d, assign, n_clusters, centroids, counts, ws, (hipStream_t)stream),
                    "rr_cluster_means");
}

size_t rr_flat_search_workspace_bytes(int k) { return rr_flat_search_workspace_bytes_for(k, rr::kMaxDim); }   // any dim
size_t rr_flat_search_workspace_bytes_for(int k, int dim) {
  if (k < 1 || k > rr::kMaxK || rr::scan_padded_dim(dim) != dim) return 0;
  const int grid = device_cus();
  return grid > 0 ? carve(nullptr, k, grid, RR_DTYPE_F16, dim).total : 0;
}

int rr_flat_search(const void* xb, int dtype, int64_t n_rows, int dim, const void* xq, int nq, int k, float* D,
                   int64_t* I, int64_t id_offset, void* ws, size_t ws_bytes, const uint8_t* route_mask,
                   int64_t mask_stride, void* stream) {
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_flat_search: bad dtype%s");
  return flat_search_impl(xb, dtype, n_rows, dim, xq, nq, k, D, I, id_offset, ws, ws_bytes, route_mask, mask_stride, nullptr, stream);
}

int rr_flat_search_l2(const void* xb, const float* half_sqnorm, int dtype, int64_t n_rows, int dim, const void* xq, int nq, int k,
                      float* D, int64_t* I, int64_t id_offset, void* ws, size_t ws_bytes, const uint8_t* route_mask,
                      int64_t mask_stride, void* stream) {
  if (!half_sqnorm && n_rows > 0) return fail(RR_ERR_INVALID, "rr_flat_search_l2: null half_sqnorm%s");
  // an empty index has no norms to pass; any non-null marker selects the L2 finalize (padding +inf) and is never dereferenced
  static const float kEmpty = 0.f;
  return flat_search_impl(xb, dtype, n_rows, dim, xq, nq, k, D, I, id_offset, ws, ws_bytes, route_mask, mask_stride,
                          half_sqnorm ? half_sqnorm : &kEmpty, stream);
}

// Validate a segment table and fill the scan's host-side description of it.  `who` names the entry point in the messages.
static int seg_host_from(const rr_segment* segs, int n_segs, int64_t n_rows_total, const uint8_t* route_mask, int64_t mask_stride,
                         const char* who, rr::SegHost& h, int64_t& scanned) {
  if (n_segs < 1 || n_segs > RR_MAX_SEGMENTS || !segs) return fail(RR_ERR_INVALID, "%s: need 1 .. 32 segments", who);
  if (n_rows_total < 0 || n_rows_total > 0xFFFFFFE0ll) return fail(RR_ERR_INVALID, "%s: bad total row count", who);
  memset(&h, 0, sizeof(h));
  h.n = (uint32_t)n_segs;
  int64_t prev_end = 0;
  int max_col = -1;
  for (int s = 0; s < n_segs; ++s) {
    const rr_segment& g = segs[s];
    // (row_begin <= n_rows_total is checked first, so the subtraction cannot overflow whatever n_rows is)
    if (g.n_rows < 0 || g.row_begin < prev_end || g.row_begin % RR_SEGMENT_ALIGN != 0 || g.row_begin > n_rows_total ||
        g.n_rows > n_rows_total - g.row_begin)
      return fail(RR_ERR_INVALID, "%s: segments must be ascending, non-overlapping, inside the matrix, and begin at "
                                  "multiples of 256 rows", who);
    if (g.mask_col < -1) return fail(RR_ERR_INVALID, "%s: mask_col must be >= -1", who);
    prev_end = g.row_begin + g.n_rows;
    if (g.mask_col > max_col) max_col = g.mask_col;
    h.row_begin[s] = (uint32_t)g.row_begin;
    h.row_limit[s] = (uint32_t)prev_end;
    h.mask_col[s] = route_mask ? g.mask_col : -1;
    h.id_offset[s] = g.id_offset;
  }
  if (route_mask && max_col >= 0 && mask_stride <= max_col)
    return fail(RR_ERR_INVALID, "%s: mask_stride must exceed every mask_col", who);
  // segment s owns the tiles up to the next segment's first row (its alignment gap included); the last one runs to the end of
  // the rows that are scanned at all: nothing behind the last valid row is read
  scanned = prev_end;
  for (int s = 0; s < n_segs; ++s) {
    const int64_t next = s + 1 < n_segs ? segs[s + 1].row_begin : scanned;
    h.tile_end[s] = (uint32_t)((next + rr::kTileRows - 1) / rr::kTileRows);
  }
  return RR_OK;
}

int rr_flat_search_segments(const void* xb, int dtype, int64_t n_rows_total, int dim, const rr_segment* segs, int n_segs,
                            const void* xq, int nq, int k, float* D, int64_t* I, void* ws, size_t ws_bytes,
                            const uint8_t* route_mask, int64_t mask_stride, void* stream) {
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_flat_search_segments: bad dtype%s");
  rr::SegHost h;
  int64_t scanned = 0;
  if (int rc = seg_host_from(segs, n_segs, n_rows_total, route_mask, mask_stride, "rr_flat_search_segments", h, scanned)) return rc;
  return flat_search_impl(xb, dtype, scanned, dim, xq, nq, k, D, I, 0, ws, ws_bytes, route_mask, mask_stride, nullptr, stream, &h);
}

int rr_flat_search_segments_l2(const void* xb, const float* half_sqnorm, int dtype, int64_t n_rows_total, int dim, const rr_segment* segs,
                               int n_segs, const void* xq, int nq, int k, float* D, int64_t* I, void* ws, size_t ws_bytes,
                               const uint8_t* route_mask, int64_t mask_stride, void* stream) {
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_flat_search_segments_l2: bad dtype%s");
  rr::SegHost h;
  int64_t scanned = 0;
  if (int rc = seg_host_from(segs, n_segs, n_rows_total, route_mask, mask_stride, "rr_flat_search_segments_l2", h, scanned)) return rc;
  if (int rc = check_search_sizes(dtype, scanned, dim, nq, k)) return rc;
  if (nq == 0) return RR_OK;
  if (!half_sqnorm && scanned > 0) return fail(RR_ERR_INVALID, "rr_flat_search_segments_l2: null half_sqnorm%s");
  // a federation without rows has no norms to pass; any non-null marker selects the L2 finalize (padding +inf), never dereferenced
  static const float kEmpty = 0.f;
  return flat_search_impl(xb, dtype, scanned, dim, xq, nq, k, D, I, 0, ws, ws_bytes, route_mask, mask_stride,
                          half_sqnorm ? half_sqnorm : &kEmpty, stream, &h);
}

// ---- f32-faithful exact search -----------------------------------------------------------------------------------------
static rr::FaithSegs faith_segs(const rr::SegHost& h) {
  rr::FaithSegs f;
  memset(&f, 0, sizeof(f));
  f.n = h.n;
  for (uint32_t s = 0; s < h.n; ++s) {
    f.row_begin[s] = h.row_begin[s];
    f.row_limit[s] = h.row_limit[s];
    f.mask_col[s] = h.mask_col[s];
    f.id_offset[s] = h.id_offset[s];
  }
  return f;
}

int rr_faithful_build(const float* xf32, int64_t ld_f32, const void* xb, int dtype, int64_t n_rows, int d, int dim, float* stats,
                      void* stream) {
  if (n_rows < 0 || d < 1 || d > dim || ld_f32 < d || rr::scan_padded_dim(dim) != dim || !stats || ((!xf32 || !xb) && n_rows > 0))
    return fail(RR_ERR_INVALID, "rr_faithful_build: bad arguments%s");
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_faithful_build: bad dtype%s");
  return hip_status(rr::launch_faithful_build(xf32, ld_f32, xb, dtype, n_rows, d, dim, (uint32_t*)stats, (hipStream_t)stream), "rr_faithful_build");
}

struct FaithWs { float* eps; float* PL; int64_t* IL; char* inner; size_t inner_bytes, total; };
static FaithWs carve_faithful(char* base, int list_len, int nq, int dim, int grid, int eps_words = 1) {
  FaithWs w;
  Bump b{base};
  w.eps = b.take<float>((size_t)nq * eps_words);
  w.PL = b.take<float>((size_t)nq * list_len);
  w.IL = b.take<int64_t>((size_t)nq * list_len);
  w.inner_bytes = carve(nullptr, list_len, grid, RR_DTYPE_F16, dim).total;
  w.inner = b.take<char>(w.inner_bytes);
  w.total = b.off;
  return w;
}

static size_t faithful_workspace_bytes(int k, int list_len, int nq, int dim, int eps_words) {
  if (k < 1 || list_len < k || list_len > rr::kMaxK || nq < 0 || rr::scan_padded_dim(dim) != dim) return 0;
  const int grid = device_cus();
  return grid > 0 ? carve_faithful(nullptr, list_len, nq, dim, grid, eps_words).total : 0;
}
size_t rr_flat_search_faithful_workspace_bytes(int k, int list_len, int nq, int dim) { return faithful_workspace_bytes(k, list_len, nq, dim, 1); }
size_t rr_flat_search_faithful_l2_workspace_bytes(int k, int list_len, int nq, int dim) { return faithful_workspace_bytes(k, list_len, nq, dim, 2); }

// Both metrics of the faithful search (`who` names the entry point in the messages).  l2: half_sqnorm is aligned with xb and
// bound receives (A(q), R(q)) [nq][2]; otherwise bound is eps [nq].
static int faithful_search(const char* who, bool l2, const void* xb, const float* half_sqnorm, int dtype, const float* xf32, int64_t ld_f32,
                           const float* stats, int64_t n_rows_total, int d, int dim, const rr_segment* segs, int n_segs, const void* xq,
                           const float* xq_f32, int nq, int k, int list_len, float* D, int64_t* I, uint8_t* exact, float* bound, void* ws,
                           size_t ws_bytes, const uint8_t* route_mask, int64_t mask_stride, void* stream) {
  using namespace rr;
  hipStream_t st = (hipStream_t)stream;
  if (!half_dtype(dtype)) return fail(RR_ERR_INVALID, "%s: bad dtype", who);
  if (k < 1 || list_len < k || list_len > kMaxK) return fail(RR_ERR_INVALID, "%s: need 1 <= k <= list_len <= 1024", who);
  if (scan_padded_dim(dim) != dim) return fail(RR_ERR_UNSUPPORTED, "%s: dim must equal rr_padded_dim(d)", who);
  if (d < 1 || d > dim || ld_f32 < d || nq < 0) return fail(RR_ERR_INVALID, "%s: bad sizes", who);
  SegHost h;
  int64_t scanned = 0;
  if (int rc = seg_host_from(segs, n_segs, n_rows_total, route_mask, mask_stride, who, h, scanned)) return rc;
  if (nq == 0) return RR_OK;
  if (!xq || !xq_f32 || !D || !I || !exact || !ws || !stats || ((!xb || !xf32) && scanned > 0)) return fail(RR_ERR_INVALID, "%s: null pointer", who);
  if (l2 && !half_sqnorm && scanned > 0) return fail(RR_ERR_INVALID, "%s: null half_sqnorm", who);
  const int grid = device_cus();
  if (grid <= 0) return fail(RR_ERR_HIP, "%s: no HIP device", who);
  FaithWs w = carve_faithful((char*)ws, list_len, nq, dim, grid, l2 ? 2 : 1);
  if (ws_bytes < w.total)
    return fail(RR_ERR_WORKSPACE, l2 ? "rr_flat_search_faithful_l2: workspace smaller than rr_flat_search_faithful_l2_workspace_bytes%s"
                                     : "rr_flat_search_faithful: workspace smaller than rr_flat_search_faithful_workspace_bytes%s");
  char where[96];
  float* e_out = bound ? bound : w.eps;
  snprintf(where, sizeof(where), "%s/queries", who);
  if (int rc = hip_status(l2 ? launch_faithful_queries_l2(xq_f32, xq, dtype, nq, d, dim, (const uint32_t*)stats, e_out, st)
                             : launch_faithful_queries(xq_f32, xq, dtype, nq, d, dim, (const uint32_t*)stats, e_out, st), where)) return rc;
  // the half rows through the ordinary segmented scan at k' = list_len, listing MATRIX rows (id_offset := row_begin)
  const FaithSegs fs = faith_segs(h);
  for (uint32_t s = 0; s < h.n; ++s) h.id_offset[s] = h.row_begin[s];
  // (a federation without rows has no norms to pass; any non-null marker selects the L2 finalize, never dereferenced)
  static const float kEmpty = 0.f;
  const float* hn = l2 ? (half_sqnorm ? half_sqnorm : &kEmpty) : nullptr;
  if (int rc = flat_search_impl(xb, dtype, scanned, dim, xq, nq, list_len, w.PL, w.IL, 0, w.inner, w.inner_bytes, route_mask, mask_stride,
                                hn, stream, &h)) return rc;
  snprintf(where, sizeof(where), "%s/rescore", who);
  return hip_status(launch_faithful_rescore(l2, xf32, ld_f32, d, xq_f32, nq, list_len, w.PL, w.IL, e_out, k, fs, route_mask, mask_stride, D, I,
                                            exact, st), where);
}

int rr_flat_search_faithful(const void* xb, int dtype, const float* xf32, int64_t ld_f32, const float* stats, int64_t n_rows_total,
                            int d, int dim, const rr_segment* segs, int n_segs, const void* xq, const float* xq_f32, int nq, int k,
                            int list_len, float* D, int64_t* I, uint8_t* exact, float* eps, void* ws, size_t ws_bytes,
                            const uint8_t* route_mask, int64_t mask_stride, void* stream) {
  return faithful_search("rr_flat_search_faithful", false, xb, nullptr, dtype, xf32, ld_f32, stats, n_rows_total, d, dim, segs, n_segs, xq, xq_f32,
                         nq, k, list_len, D, I, exact, eps, ws, ws_bytes, route_mask, mask_stride, stream);
}

int rr_flat_search_faithful_l2(const void* xb, const float* half_sqnorm, int dtype, const float* xf32, int64_t ld_f32, const float* stats,
                               int64_t n_rows_total, int d, int dim, const rr_segment* segs, int n_segs, const void* xq, const float* xq_f32,
                               int nq, int k, int list_len, float* D, int64_t* I, uint8_t* exact, float* bound, void* ws, size_t ws_bytes,
                               const uint8_t* route_mask, int64_t mask_stride, void* stream) {
  return faithful_search("rr_flat_search_faithful_l2", true, xb, half_sqnorm, dtype, xf32, ld_f32, stats, n_rows_total, d, dim, segs, n_segs, xq,
                         xq_f32, nq, k, list_len, D, I, exact, bound, ws, ws_bytes, route_mask, mask_stride, stream);
}

// exact scan: per block of queries [G][k] lists -> (two-level if G*k > 8192) merge -> [k] -> D / I rows
struct ExactWs { float *D1, *D2, *D3; int64_t *I1, *I2, *I3; size_t total; };
static ExactWs carve_exact(char* base, const rr::FaithPlan& p, int k) {
  ExactWs w;
  Bump b{base};
  const size_t l1 = (size_t)p.nqb * p.G * k, l2 = (size_t)p.nqb * ((p.G + p.gs - 1) / p.gs) * k, l3 = (size_t)p.nqb * k;
  w.D1 = b.take<float>(l1); w.I1 = b.take<int64_t>(l1);
  w.D2 = b.take<float>(l2); w.I2 = b.take<int64_t>(l2);
  w.D3 = b.take<float>(l3); w.I3 = b.take<int64_t>(l3);
  w.total = b.off;
  return w;
}

size_t rr_flat_search_f32_exact_workspace_bytes(int k, int d) {
  if (k < 1 || k > rr::kMaxK || d < 1 || d > rr::kMaxDim) return 0;
  const int grid = device_cus();
  return grid > 0 ? carve_exact(nullptr, rr::faithful_plan(k, d, grid, -1), k).total : 0;
}

// l2: rows are keyed by -D, so the descending merges below list the nearest first; the emit kernel turns the keys back into distances
static int f32_exact_search(const char* who, bool l2, const float* xf32, int64_t ld_f32, int64_t n_rows_total, int d, const rr_segment* segs,
                            int n_segs, const float* xq_f32, int nq, const int32_t* qidx, int n_idx, int k, float* D, int64_t* I, void* ws,
                            size_t ws_bytes, const uint8_t* route_mask, int64_t mask_stride, void* stream) {
  using namespace rr;
  hipStream_t st = (hipStream_t)stream;
  if (k < 1 || k > kMaxK) return fail(RR_ERR_INVALID, "%s: k must be in [1, 1024]", who);
  if (d < 1 || d > kMaxDim || ld_f32 < d || nq < 0 || n_idx < 0 || (!qidx && n_idx > nq)) return fail(RR_ERR_INVALID, "%s: bad sizes", who);
  SegHost h;
  int64_t scanned = 0;
  if (int rc = seg_host_from(segs, n_segs, n_rows_total, route_mask, mask_stride, who, h, scanned)) return rc;
  if (n_idx == 0) return RR_OK;
  if (!xq_f32 || !D || !I || !ws || (!xf32 && scanned > 0)) return fail(RR_ERR_INVALID, "%s: null pointer", who);
  const int grid = device_cus();
  if (grid <= 0) return fail(RR_ERR_HIP, "%s: no HIP device", who);
  const FaithPlan p = faithful_plan(k, d, grid, scanned);
  ExactWs w = carve_exact((char*)ws, p, k);
  if (ws_bytes < w.total) return fail(RR_ERR_WORKSPACE, "%s: workspace smaller than rr_flat_search_f32_exact_workspace_bytes", who);
  const FaithSegs fs = faith_segs(h);
  char where[96];
  const auto at = [&](const char* step) { snprintf(where, sizeof(where), "%s/%s", who, step); return (const char*)where; };
  for (int q0 = 0; q0 < n_idx; q0 += p.nqb) {
    const int nqb = n_idx - q0 < p.nqb ? n_idx - q0 : p.nqb;
    if (int rc = hip_status(launch_faithful_scan(l2, p, xf32, ld_f32, d, scanned, xq_f32, qidx, q0, nqb, k, fs, route_mask, mask_stride, w.D1, w.I1, st),
                            at("scan"))) return rc;
    const float* Dm = w.D1;
    const int64_t* Im = w.I1;
    int lists = p.G;
    if (lists > p.gs) {   // level 1: groups of gs consecutive lists of one query -> [nqb][G / gs][k]
      const MergeSrc src{w.D1, w.I1, p.gs * k, 1, 0, 0, 0};
      if (int rc = hip_status(launch_merge_topk(src, nqb * (lists / p.gs), p.gs * k, k, 1, w.D2, w.I2, st), at("merge1"))) return rc;
      Dm = w.D2; Im = w.I2; lists /= p.gs;
    }
    const MergeSrc src{Dm, Im, lists * k, 1, 0, 0, 0};
    if (int rc = hip_status(launch_merge_topk(src, nqb, lists * k, k, 1, w.D3, w.I3, st), at("merge"))) return rc;
    if (int rc = hip_status(launch_faithful_emit(l2, w.D3, w.I3, qidx, q0, nqb, k, fs, D, I, st), at("emit"))) return rc;
  }
  return RR_OK;
}

int rr_flat_search_f32_exact(const float* xf32, int64_t ld_f32, int64_t n_rows_total, int d, const rr_segment* segs, int n_segs,
                             const float* xq_f32, int nq, const int32_t* qidx, int n_idx, int k, float* D, int64_t* I, void* ws,
                             size_t ws_bytes, const uint8_t* route_mask, int64_t mask_stride, void* stream) {
  return f32_exact_search("rr_flat_search_f32_exact", false, xf32, ld_f32, n_rows_total, d, segs, n_segs, xq_f32, nq, qidx, n_idx, k, D, I, ws,
                          ws_bytes, route_mask, mask_stride, stream);
}

int rr_flat_search_f32_exact_l2(const float* xf32, int64_t ld_f32, int64_t n_rows_total, int d, const rr_segment* segs, int n_segs,
                                const float* xq_f32, int nq, const int32_t* qidx, int n_idx, int k, float* D, int64_t* I, void* ws,
                                size_t ws_bytes, const uint8_t* route_mask, int64_t mask_stride, void* stream) {
  return f32_exact_search("rr_flat_search_f32_exact_l2", true, xf32, ld_f32, n_rows_total, d, segs, n_segs, xq_f32, nq, qidx, n_idx, k, D, I, ws,
                          ws_bytes, route_mask, mask_stride, stream);
}

// ---- int8 screening copy ---------------------------------------------------------------------------------
struct ScreenWs { int8_t* q8; float* qinfo; float* PL; int64_t* IL; char* inner; size_t inner_bytes, total; };
static ScreenWs carve_screen(char* base, int list_len, int nq, int dim8, int grid) {
  ScreenWs w;
  Bump b{base};
  w.q8 = b.take<int8_t>((size_t)nq * dim8);
  w.qinfo = b.take<float>((size_t)nq * 2);
  w.PL = b.take<float>((size_t)nq * list_len);
  w.IL = b.take<int64_t>((size_t)nq * list_len);
  w.inner_bytes = carve(nullptr, list_len, grid, rr::kDtypeI8, dim8 / 2).total;
  w.inner = b.take<char>(w.inner_bytes);
  w.total = b.off;
  return w;
}

int rr_screen_dim(int dim) {
  if (dim < 8 || dim % 8 != 0) return RR_ERR_INVALID;
  const int d8 = (dim + 255) / 256 * 256;
  return d8 <= 2 * rr::kMaxResidentDim ? d8 : RR_ERR_UNSUPPORTED;
}

int rr_screen_build(const void* xb, int dtype, int64_t n_rows, int dim, void* x8, float* stats, void* stream) {
  const int dim8 = rr_screen_dim(dim);
  if (dim8 < 0) return fail(dim8, "rr_screen_build: the int8 screening copy needs dim <= 1536, a multiple of 8%s");
  if (n_rows < 0 || !stats || ((!xb || !x8) && n_rows > 0)) return fail(RR_ERR_INVALID, "rr_screen_build: bad arguments%s");
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_screen_build: bad dtype%s");
  return hip_status(rr::launch_screen_build(xb, dtype, n_rows, dim, (int8_t*)x8, dim8, (uint32_t*)stats, (hipStream_t)stream), "rr_screen_build");
}

size_t rr_flat_search_screened_workspace_bytes(int k, int list_len, int nq, int dim) {
  const int dim8 = rr_screen_dim(dim);
  if (k < 1 || list_len < k || list_len > rr::kMaxK || nq < 0 || dim8 < 0) return 0;
  const int grid = device_cus();
  return grid > 0 ? carve_screen(nullptr, list_len, nq, dim8, grid).total : 0;
}

int rr_flat_search_screened(const void* xb, int dtype, const void* x8, const float* stats, int64_t n_rows, int dim, const void* xq,
                            int nq, int k, int list_len, float* D, int64_t* I, int64_t id_offset, uint8_t* exact, void* ws,
                            size_t ws_bytes, const uint8_t* route_mask, int64_t mask_stride, void* stream) {
  using namespace rr;
  hipStream_t st = (hipStream_t)stream;
  const int dim8 = rr_screen_dim(dim);
  if (dim8 < 0) return fail(RR_ERR_UNSUPPORTED, "rr_flat_search_screened: dim must be a multiple of 8, <= 1536%s");
  if (k < 1 || list_len < k || list_len > kMaxK) return fail(RR_ERR_INVALID, "rr_flat_search_screened: need 1 <= k <= list_len <= 1024%s");
  if (!half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_flat_search_screened: bad dtype%s");
  if (nq < 0 || n_rows < 0) return fail(RR_ERR_INVALID, "rr_flat_search_screened: negative size%s");
  if (nq == 0) return RR_OK;
  if (!xq || !D || !I || !exact || !ws || !stats || ((!xb || !x8) && n_rows > 0))
    return fail(RR_ERR_INVALID, "rr_flat_search_screened: null pointer%s");
  const int grid = device_cus();
  if (grid <= 0) return fail(RR_ERR_HIP, "rr_flat_search_screened: no HIP device%s");
  ScreenWs w = carve_screen((char*)ws, list_len, nq, dim8, grid);
  if (ws_bytes < w.total) return fail(RR_ERR_WORKSPACE, "rr_flat_search_screened: workspace smaller than rr_flat_search_screened_workspace_bytes%s");
  if (int rc = hip_status(launch_screen_queries(xq, dtype, nq, dim, w.q8, dim8, (const uint32_t*)stats, w.qinfo, st),
                          "rr_flat_search_screened/queries")) return rc;
  // the int8 rows through the same scan + exact selection, k' = list_len; a row of dim8 bytes is dim8/2 two-byte elements
  if (int rc = flat_search_impl(x8, kDtypeI8, n_rows, dim8 / 2, w.q8, nq, list_len, w.PL, w.IL, 0, w.inner, w.inner_bytes, nullptr, 0, nullptr,
                                stream)) return rc;
  return hip_status(launch_rescore(xb, xq, dtype, dim, nq, list_len, w.PL, w.IL, w.qinfo, k, D, I, id_offset, exact, route_mask, mask_stride, st),
                    "rr_flat_search_screened/rescore");
}

int rr_half_sqnorms(const void* xb, int dtype, int64_t n_rows, int dim, float* out, void* stream) {
  if (n_rows < 0 || dim < 8 || dim % 8 != 0 || ((!xb || !out) && n_rows > 0)) return fail(RR_ERR_INVALID, "rr_half_sqnorms: bad arguments%s");
  if (!rr::half_dtype(dtype)) return fail(RR_ERR_INVALID, "rr_half_sqnorms: bad dtype%s");
  return hip_status(rr::launch_half_sqnorms(xb, dtype, n_rows, dim, out, (hipStream_t)stream), "rr_half_sqnorms");
}

int rr_profile_begin(int max_launches) {
  if (g_prof) return fail(RR_ERR_INVALID, "rr_profile_begin: already profiling%s");
  if (max_launches < 1) return fail(RR_ERR_INVALID, "rr_profile_begin: max_launches < 1%s");
  g_prof = new ProfEntry[max_launches];
  g_prof_cap = 0;
  g_prof_n = 0;
  g_prof_dropped = 0;
  for (int i = 0; i < max_launches; ++i) {
    if (hipEventCreate(&g_prof[i].start) != hipSuccess || hipEventCreate(&g_prof[i].stop) != hipSuccess)
      return fail(RR_ERR_HIP, "rr_profile_begin: hipEventCreate failed%s");
    g_prof_cap = i + 1;
  }
  return RR_OK;
}

int rr_profile_end(double* scan_ms_total, int* n_launches, double* rows_scanned) {
  if (!g_prof) return fail(RR_ERR_INVALID, "rr_profile_end: not profiling%s");
  double ms = 0, rows = 0;
  int n = 0;
  for (int i = 0; i < g_prof_n; ++i) {
    float t = 0;
    if (hipEventSynchronize(g_prof[i].stop) == hipSuccess && hipEventElapsedTime(&t, g_prof[i].start, g_prof[i].stop) == hipSuccess) {
      ms += t; rows += (double)g_prof[i].rows; ++n;
    }
  }
  for (int i = 0; i < g_prof_cap; ++i) { (void)hipEventDestroy(g_prof[i].start); (void)hipEventDestroy(g_prof[i].stop); }
  delete[] g_prof;
  g_prof = nullptr;
  g_prof_cap = g_prof_n = 0;
  if (scan_ms_total) *scan_ms_total = ms;
  if (n_launches) *n_launches = n;
  if (rows_scanned) *rows_scanned = rows;
  if (g_prof_dropped > 0) {
    char msg[32];
    snprintf(msg, sizeof(msg), "%d", g_prof_dropped);
    g_prof_dropped = 0;
    return fail(RR_ERR_WORKSPACE, "rr_profile_end: %s scan launches were not recorded (max_launches of rr_profile_begin too small); the totals returned are incomplete", msg);
  }
  return RR_OK;
}

const char* rr_flat_scan_kernel_name(int dim, int nq) {
  if (rr::scan_padded_dim(dim) != dim || nq < 1) return "";
  return rr::scan_plan(RR_DTYPE_F16, dim, nq > rr::kQueriesPerBlock ? rr::kQueriesPerBlock : nq, false).name;
}

int rr_merge_topk(const float* Din, const int64_t* Iin, int nq, int m, int k, int descending, float* Dout,
                  int64_t* Iout, void* stream) {
  if (nq < 0 || m < 0 || k < 1) return fail(RR_ERR_INVALID, "rr_merge_topk: bad sizes%s");
  if (m > rr::kSelectCap) return fail(RR_ERR_UNSUPPORTED, "rr_merge_topk: m > 8192 candidates per query%s");
  if (nq == 0) return RR_OK;
  if ((m > 0 && (!Din || !Iin)) || !Dout || !Iout) return fail(RR_ERR_INVALID, "rr_merge_topk: null pointer%s");
  const rr::MergeSrc src{Din, Iin, m > 0 ? m : 1, 1, 0, 0, 0};
  return hip_status(rr::launch_merge_topk(src, nq, m, k, descending, Dout, Iout, (hipStream_t)stream), "rr_merge_topk");
}

int rr_merge_topk_gathered(const void* gathered, int n_ranks, size_t rank_stride_bytes, size_t ids_offset_bytes, int slots, int nq,
                           int k_in, int k, int descending, float* Dout, int64_t* Iout, void* stream) {
  if (n_ranks < 1 || slots < 1 || nq < 0 || k_in < 1 || k < 1) return fail(RR_ERR_INVALID, "rr_merge_topk_gathered: bad sizes%s");
  const size_t list_elems = (size_t)nq * k_in;
  if (rank_stride_bytes % 8 != 0 || ids_offset_bytes % 8 != 0 || ids_offset_bytes < (size_t)slots * list_elems * 4 ||
      rank_stride_bytes < ids_offset_bytes + (size_t)slots * list_elems * 8)
    return fail(RR_ERR_INVALID, "rr_merge_topk_gathered: the rank stride / id offset do not describe [D f32[slots][nq][k_in] | pad | I i64[slots][nq][k_in]]%s");
  const long long m = (long long)n_ranks * slots * k_in;
  if (m > rr::kSelectCap) return fail(RR_ERR_UNSUPPORTED, "rr_merge_topk_gathered: more than 8192 candidates per query%s");
  if (nq == 0) return RR_OK;
  if (!gathered || !Dout || !Iout) return fail(RR_ERR_INVALID, "rr_merge_topk_gathered: null pointer%s");
  if ((uintptr_t)gathered % 8 != 0) return fail(RR_ERR_INVALID, "rr_merge_topk_gathered: the buffer must be 8-byte aligned%s");
  const rr::MergeSrc src{(const float*)gathered, (const int64_t*)((const char*)gathered + ids_offset_bytes), k_in, slots,
                         (int64_t)(rank_stride_bytes / 4), (int64_t)(rank_stride_bytes / 8), (int64_t)list_elems};
  return hip_status(rr::launch_merge_topk(src, nq, (int)m, k, descending, Dout, Iout, (hipStream_t)stream), "rr_merge_topk_gathered");
}

static bool router_header_ok(const rr_router_weights* w) {
  // d_max: the widest embedding EVERY batch size can be served at (the small-batch kernel's LDS, rr_kernels.h)
  return w && w->n_sources >= 1 && w->d_max >= 1 && w->n_models >= 1 && w->d_max <= rr::kRouterMaxDmax;
}
// Argument validation of the router entry points; `who` names the entry point in the messages.  nq == 0 needs no buffers.
static int router_check(const rr_router_weights* w, const float* xq, int nq, float* logits, uint8_t* mask, const char* who) {
  if (!w || nq < 0) return fail(RR_ERR_INVALID, "%s: bad arguments", who);
  if (!router_header_ok(w)) return fail(RR_ERR_INVALID, "%s: bad weight header (n_sources, n_models >= 1, d_max 1 ... 8191)", who);
  if (nq > 0 && (!xq || !logits || !mask || !w->w1q || !w->c1 || !w->w2 || !w->w3 || !w->model_of_source))
    return fail(RR_ERR_INVALID, "%s: null pointer", who);
  return RR_OK;
}

int rr_router_mlp(const rr_router_weights* w, const float* xq, int nq, float* logits, uint8_t* mask, void* stream) {
  if (int rc = router_check(w, xq, nq, logits, mask, "rr_router_mlp")) return rc;
  if (nq == 0) return RR_OK;
  return hip_status(rr::launch_router_mlp(w, xq, nq, logits, mask, (hipStream_t)stream), "rr_router_mlp");
}

size_t rr_router_workspace_bytes(const rr_router_weights* w, int nq) {
  return nq >= 0 && router_header_ok(w) ? rr::router_workspace_bytes(w, nq) : 0;
}

int rr_router_mlp_ws(const rr_router_weights* w, const float* xq, int nq, float* logits, uint8_t* mask, void* ws, size_t ws_bytes,
                     void* stream) {
  if (int rc = router_check(w, xq, nq, logits, mask, "rr_router_mlp_ws")) return rc;
  if (nq == 0) return RR_OK;
  const size_t need = rr::router_workspace_bytes(w, nq);
  if (need == 0)  // small batch: the latency-oriented kernel, no workspace
    return rr_router_mlp(w, xq, nq, logits, mask, stream);
  if (!ws || ws_bytes < need) return fail(RR_ERR_WORKSPACE, "rr_router_mlp_ws: workspace smaller than rr_router_workspace_bytes%s");
  return hip_status(rr::launch_router_mlp_ws(w, xq, nq, logits, mask, ws, (hipStream_t)stream), "rr_router_mlp_ws");
}

}  // extern "C"
