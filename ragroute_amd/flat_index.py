"""faiss-shaped flat index whose corpus lives in HBM and whose search is the HIP scan kernel.

Mirrors the operator surface the reference uses from `faiss` (ragroute/data_source.py):
  index.search(xq: float32[nq,d], k) -> (D float32[nq,k], I int64[nq,k])      data_source.py:158,186,203
  index.ntotal, index.d
  normalize_L2(x: float32[n,d])  in place                                       data_source.py:198-199
PyTorch is used for device memory and streams only; all arithmetic is in libragroute_hip.so (reached through _calls.py).
"""
import numpy as np
import torch

from . import _calls
from . import _lib
from ._lib import check, lib

_K_RANGE = f"k must be in [1, {_lib.RR_MAX_K}], got {{0}}"
_LIST_RANGE = f"need 1 <= k <= list_len <= {_lib.RR_MAX_K}, got k={{0}}, list_len={{1}}"


def normalize_L2(x):
    """In-place row-wise L2 normalisation (faiss.normalize_L2, data_source.py:198-199).
    Accepts a C-contiguous float32 numpy array [n,d] (normalised in place through the GPU) or a
    float32 CUDA tensor (normalised in place on device)."""
    if isinstance(x, torch.Tensor):
        if x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous() or x.dim() != 2:
            raise ValueError("normalize_L2 needs a contiguous float32 CUDA tensor [n,d]")
        _calls.l2_normalize_(x)
        return
    if not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.ndim == 2 and x.flags.c_contiguous):
        raise ValueError("normalize_L2 needs a C-contiguous float32 array [n,d]")
    _calls.require_gpu()
    t = torch.from_numpy(x).cuda()
    _calls.l2_normalize_(t)
    x[...] = t.cpu().numpy()


class _Index:
    """What FlatIndex and SegmentedIndex share: the dimensions, metric, dtype and device, the query preparation, the scan workspace,
    the half-precision search of a half matrix `_xb` (with `_hn`, its half squared norms, under "l2") and the f32-faithful mode.
    A subclass owns the storage and says what differs: `_segments()`, its segment table; `_n_rows`, the matrix rows it scans;
    `_mask_args()`, the check of its route mask (a vector per index, a matrix per segmented one).

    The f32-faithful mode (exact_f32=True; C ABI rr_flat_search_faithful; under the squared-L2 metric exact_l2=True and
    rr_flat_search_faithful_l2, which also reads `_hn`): the f32 rows `_xf` beside the half copy `_xb`, their error / norm maxima
    `_fstats`, and the search that proves every query's top-k on the f32 rows — a query whose proof fails is repeated with a list
    of 1024 rows (`faithful_retries` counts those queries), and what is still unproven is answered by the exact f32 scan
    (`faithful_fallbacks`)."""

    def __init__(self, d, metric, dtype, device, exact_f32, exact_l2):
        if metric not in ("ip", "cosine", "l2"):
            raise ValueError(f"unknown metric {metric!r}")
        if exact_f32 and metric == "l2":
            raise ValueError("exact_f32 serves the ip / cosine metrics only")
        if exact_l2 and metric != "l2":
            raise ValueError("exact_l2 serves the l2 metric only (ip / cosine: exact_f32)")
        if dtype not in _calls.TORCH_DTYPE:
            raise ValueError(f"unknown dtype {dtype!r}")
        self.d = int(d)
        self.metric = metric
        self.dtype = dtype
        self.dim = lib().rr_padded_dim(self.d)
        if self.dim < 0:
            raise _lib.RagrouteHipError(f"embedding dimension {d} is not supported (max 8192)")
        _calls.require_gpu()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.exact_f32 = bool(exact_f32)
        self.exact_l2 = bool(exact_l2)
        self._hn = None  # |x|^2/2 per matrix row (metric "l2")
        self._ws = {}

    @property
    def _faith(self):
        return self.exact_f32 or self.exact_l2

    def _faithful_init(self, n_rows):
        if not self._faith:
            return
        self._xf = torch.zeros((max(1, n_rows), self.d), dtype=torch.float32, device=self.device)
        self._fstats = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._ws_faithful = {}
        self._ws_exact = {}
        self.faithful_list = None   # rows re-scored per query; None = min(1024, max(256, 4 k))
        self.faithful_retries = 0
        self.faithful_fallbacks = 0

    # -- ingest ------------------------------------------------------------------------------
    def _ingest(self, x, row0, chunk_rows):
        """f32 rows (numpy, np.memmap or tensor) -> matrix rows [row0, row0 + n) of the half copy, normalised for cosine.  Faithful: the
        f32 rows go to `_xf` first (normalised by rr_l2_normalize_f32) and the half copy is derived from what lies there."""
        for s in range(0, x.shape[0], chunk_rows):
            part = _calls.f32_rows(x[s: s + chunk_rows], self.device)
            lo, hi = row0 + s, row0 + s + part.shape[0]
            if self._faith:
                f = self._xf[lo:hi]
                f.copy_(part)
                if self.metric == "cosine":
                    _calls.l2_normalize_(f)
                _calls.rows_to_half(f, self.dim, self._xb.dtype, False, self._xb[lo:hi])
            else:
                _calls.rows_to_half(part, self.dim, self._xb.dtype, self.metric == "cosine", self._xb[lo:hi])
            del part   # before the next chunk is staged

    def _faithful_build(self):
        """Faithful: the maxima over the whole matrix."""
        if self._faith:
            check(lib().rr_faithful_build(self._xf.data_ptr(), self.d, self._xb.data_ptr(), _calls.RR_DTYPE[self.dtype], self._n_rows, self.d,
                                          self.dim, self._fstats.data_ptr(), _calls.stream_ptr()), "rr_faithful_build")

    # -- queries, workspace, the half-precision search ------------------------------------------
    def prepare_queries(self, xq):
        """float32 [nq,d] (numpy or tensor) -> device [nq,dim] in the index dtype (normalised for cosine).
        exact_f32 / exact_l2: the pair (half [nq,dim], f32 [nq,d]) that search_prepared() takes (both normalised for cosine)."""
        xf = _calls.f32_queries(xq, self.d, self.device)
        if not self._faith:
            return _calls.rows_to_half(xf, self.dim, self._xb.dtype, self.metric == "cosine")
        if self.metric == "cosine":
            xf = xf.clone()
            _calls.l2_normalize_(xf)
        return _calls.rows_to_half(xf, self.dim, self._xb.dtype, False), xf

    def _workspace(self, k):
        return _calls.workspace(self._ws, k, self.device, _K_RANGE, "rr_flat_search_workspace_bytes_for", k, self.dim)

    def _half_search(self, xq_half, k, route_mask, out, n_rows, id_offset=0, segs=None):
        """Checked prepared queries -> (D, I): rr_flat_search / _l2 over n_rows rows, or their segmented forms over the table `segs`."""
        nq = xq_half.shape[0]
        ws = self._workspace(k)
        D, I = _calls.out_pair(nq, k, self.device, out)
        mptr, mstride = self._mask_args(route_mask, nq)
        _calls.half_search(self._xb, n_rows, xq_half, k, D, I, ws, mptr, mstride, id_offset, segs, self.metric == "l2", self._hn)
        return D, I

    # -- the f32-faithful search ---------------------------------------------------------------
    def _faithful_list_len(self, k):
        L = self.faithful_list if self.faithful_list is not None else min(_lib.RR_MAX_K, max(256, 4 * k))
        return max(int(L), k)

    def _faithful_raw(self, xq_half, xq_f32, k, L, segs, n_rows_total, mptr, mstride, D=None, I=None):
        nq = xq_half.shape[0]
        ws = _calls.workspace(self._ws_faithful, (k, L, nq), self.device, _LIST_RANGE,
                              "rr_flat_search_faithful_l2_workspace_bytes" if self.exact_l2 else "rr_flat_search_faithful_workspace_bytes",
                              k, L, nq, self.dim)
        D, I = _calls.out_pair(nq, k, self.device, None if D is None else (D, I))
        exact = torch.empty(nq, dtype=torch.uint8, device=self.device)
        if self.exact_l2:
            bound = torch.empty((nq, 2), dtype=torch.float32, device=self.device)   # (A(q), R(q))
            check(lib().rr_flat_search_faithful_l2(self._xb.data_ptr(), self._hn.data_ptr() if self._hn is not None else None,
                                                   _calls.RR_DTYPE[self.dtype], self._xf.data_ptr(), self.d, self._fstats.data_ptr(), n_rows_total,
                                                   self.d, self.dim, segs, len(segs), xq_half.data_ptr(), xq_f32.data_ptr(), nq, k, L,
                                                   D.data_ptr(), I.data_ptr(), exact.data_ptr(), bound.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   mptr, mstride, _calls.stream_ptr()), "rr_flat_search_faithful_l2")
            return D, I, exact, bound
        eps = torch.empty(nq, dtype=torch.float32, device=self.device)
        check(lib().rr_flat_search_faithful(self._xb.data_ptr(), _calls.RR_DTYPE[self.dtype], self._xf.data_ptr(), self.d, self._fstats.data_ptr(),
                                            n_rows_total, self.d, self.dim, segs, len(segs), xq_half.data_ptr(), xq_f32.data_ptr(), nq, k, L,
                                            D.data_ptr(), I.data_ptr(), exact.data_ptr(), eps.data_ptr(), ws.data_ptr(), ws.numel(), mptr,
                                            mstride, _calls.stream_ptr()), "rr_flat_search_faithful")
        return D, I, exact, eps

    def _exact_scan(self, xq_f32, qidx, k, segs, n_rows_total, mptr, mstride, D, I):
        ws = _calls.workspace(self._ws_exact, k, self.device, _K_RANGE, "rr_flat_search_f32_exact_workspace_bytes", k, self.d)
        name = "rr_flat_search_f32_exact_l2" if self.exact_l2 else "rr_flat_search_f32_exact"
        check(getattr(lib(), name)(self._xf.data_ptr(), self.d, n_rows_total, self.d, segs, len(segs), xq_f32.data_ptr(),
                                   xq_f32.shape[0], qidx.data_ptr() if qidx is not None else None,
                                   qidx.numel() if qidx is not None else xq_f32.shape[0], k, D.data_ptr(), I.data_ptr(),
                                   ws.data_ptr(), ws.numel(), mptr, mstride, _calls.stream_ptr()), name)

    def _faithful_search(self, xq, k, route_mask, out, segs, n_rows_total):
        """search_exact_f32, then one host read of the proof flags; unproven queries again at list_len = 1024, then the exact scan."""
        if not (isinstance(xq, tuple) and len(xq) == 2):
            raise ValueError("an exact_f32 / exact_l2 index searches the (half, f32) query pair that prepare_queries() returns")
        xq_half, xq_f32 = xq
        pair = "search_prepared() needs the contiguous ([nq, dim] index dtype, [nq, d] float32) pair of prepare_queries()"
        _calls.check_half_queries(xq_half, self._xb.dtype, self.dim, pair)
        if xq_f32.dtype != torch.float32 or xq_f32.shape != (xq_half.shape[0], self.d) or not xq_f32.is_contiguous():
            raise ValueError(pair)
        nq = xq_half.shape[0]
        D, I = out if out is not None else (None, None)
        mptr, mstride = self._mask_args(route_mask, nq)
        D, I, exact, _ = self._faithful_raw(xq_half, xq_f32, k, self._faithful_list_len(k), segs, n_rows_total, mptr, mstride, D, I)
        if nq == 0:
            return D, I
        bad = torch.nonzero(exact == 0).flatten()
        if bad.numel() == 0:
            return D, I
        self.faithful_retries += int(bad.numel())
        still = bad
        if self._faithful_list_len(k) < _lib.RR_MAX_K:
            sub_mask = route_mask[bad].contiguous() if route_mask is not None else None
            smptr, smstride = self._mask_args(sub_mask, int(bad.numel()))
            D2, I2, ex2, _ = self._faithful_raw(xq_half[bad].contiguous(), xq_f32[bad].contiguous(), k, _lib.RR_MAX_K, segs, n_rows_total,
                                                smptr, smstride)
            D[bad] = D2
            I[bad] = I2
            still = bad[ex2 == 0]
        if still.numel():
            self.faithful_fallbacks += int(still.numel())
            self._exact_scan(xq_f32, still.to(torch.int32).contiguous(), k, segs, n_rows_total, mptr, mstride, D, I)
        return D, I

    def search_exact_f32(self, xq_f32_dev, k, list_len=None, route_mask=None, id_offset=0):
        """exact_f32 index, device to device, no host sync: float32 queries [nq,d] -> (D, I, exact, eps) CUDA tensors.  exact[q] == 1
        where the top-k is proven on the f32 rows; eps[q] is the bound on the half-precision scan's error for query q (an exact_l2
        index returns the bound [nq, 2] = (A(q), R(q)) in its place).  search() and search_prepared() wrap this with the retry
        and the exact fallback."""
        if not self._faith:
            raise _lib.RagrouteHipError("search_exact_f32() needs an index built with exact_f32=True or exact_l2=True")
        xh, xf = self.prepare_queries(xq_f32_dev)
        L = self._faithful_list_len(k) if list_len is None else int(list_len)
        mptr, mstride = self._mask_args(route_mask, xh.shape[0])
        return self._faithful_raw(xh, xf, int(k), L, self._segments(id_offset, route_mask), self._n_rows, mptr, mstride)

    def search(self, xq, k, route_mask=None):
        """float32 [nq,d] -> (D float32[nq,k], I int64[nq,k]) numpy arrays; route_mask (tensor or array) as search_prepared()."""
        with torch.cuda.device(self.device):
            if route_mask is not None and not isinstance(route_mask, torch.Tensor):
                route_mask = torch.from_numpy(np.ascontiguousarray(route_mask, dtype=np.uint8)).to(self.device)
            D, I = self.search_prepared(self.prepare_queries(xq), int(k), route_mask=route_mask)
            return D.cpu().numpy(), I.cpu().numpy()


class FlatIndex(_Index):
    """Exact inner-product index (the role of faiss.IndexFlatIP in the reference).

    metric: "ip" (reference behaviour), "cosine" (rows and queries L2-normalised on ingest/search, i.e. normalize_L2 + IP
    as data_source.py:196-203 does for the wikipedia corpora) or "l2" (squared L2 distances, nearest first: the role of
    faiss.IndexFlatL2).
    dtype : "fp16" or "bf16" storage/MFMA input type; scores accumulate in f32.

    build_screen() adds an int8 screening copy (ip / cosine, d <= 1536): searches then stream half the bytes and return the
    same exact top-k, proven per query by a quantisation-error bound; a batch whose proof fails is repeated on the
    f16/bf16 rows (counted in `screen_fallbacks`).

    exact_f32=True (ip / cosine): the f32 rows are kept beside the half copy (3x the half bytes) and searches return what the
    reference's IndexFlatIP returns on the UNROUNDED f32 rows and queries, bit for bit with an f64-accumulating CPU scan: the half
    copy only screens (include/ragroute_hip.h rr_flat_search_faithful).  prepare_queries() then returns a (half, f32) pair.

    exact_l2=True (l2): the same mode under the squared-L2 metric — the distances of the reference's IndexFlatL2 on the unrounded
    f32 rows and queries, nearest first (rr_flat_search_faithful_l2); everything said of an exact_f32 index holds for it.
    """

    def __init__(self, d, metric="ip", dtype="fp16", device=None, exact_f32=False, exact_l2=False):
        super().__init__(d, metric, dtype, device, exact_f32, exact_l2)
        self.ntotal = 0
        self._xb = torch.empty((0, self.dim), dtype=_calls.TORCH_DTYPE[dtype], device=self.device)
        self._x8 = self._x8_stats = None   # int8 screening copy (build_screen)
        self._ws_screen = {}
        self.screen_list = 512
        self.screen_fallbacks = 0
        self._faithful_init(0)

    @property
    def _n_rows(self):
        return self.ntotal

    def _segments(self, id_offset=0, route_mask=None):
        """The faithful modes' one-entry segment table (the plain search never goes through it)."""
        return (_lib.SegmentStruct * 1)(_lib.SegmentStruct(0, self.ntotal, int(id_offset), 0 if route_mask is not None else -1, 0))

    @staticmethod
    def _mask_args(route_mask, nq):
        if route_mask is None:
            return None, 0
        if route_mask.dtype not in (torch.bool, torch.uint8) or route_mask.dim() != 1 or route_mask.shape[0] != nq or not route_mask.is_cuda:
            raise ValueError("route_mask must be a bool/uint8 CUDA vector with one entry per query")
        return route_mask.data_ptr(), route_mask.stride(0)

    # -- storage -----------------------------------------------------------------------------
    def reserve(self, n):
        if n > self._xb.shape[0]:
            new = torch.empty((n, self.dim), dtype=self._xb.dtype, device=self.device)
            new[: self.ntotal].copy_(self._xb[: self.ntotal])
            self._xb = new
            if self._faith:
                newf = torch.empty((n, self.d), dtype=torch.float32, device=self.device)
                newf[: self.ntotal].copy_(self._xf[: self.ntotal])
                self._xf = newf

    def add(self, x, chunk_rows=1 << 18):
        """Append rows (float32 numpy [n,d] or CUDA tensor) to the HBM-resident corpus."""
        n = x.shape[0]
        if x.shape[1] != self.d:
            raise ValueError(f"expected rows of dimension {self.d}, got {x.shape[1]}")
        if self.ntotal + n > self._xb.shape[0]:
            self.reserve(max(self.ntotal + n, int(self._xb.shape[0] * 1.5)))
        with torch.cuda.device(self.device):
            self._ingest(x, self.ntotal, chunk_rows)
            self.ntotal += n
            self._faithful_build()
        self._x8 = self._x8_stats = None  # one scale for the whole corpus: the screening copy is rebuilt, not appended to
        self._refresh_norms()   # (exact_l2 too: the scan of the half copy ranks by them)

    def _refresh_norms(self):
        if self.metric != "l2":
            return
        self._hn = torch.empty(max(1, self.ntotal), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _calls.half_sqnorms(self._xb, self.ntotal, self._hn)

    def adopt(self, xb_dev, ntotal=None):
        """Use an existing device matrix [n, dim] of the index dtype as the corpus (no copy)."""
        if self._faith:
            raise _lib.RagrouteHipError("adopt() takes a half matrix only; an exact_f32 / exact_l2 index ingests its f32 rows with add()")
        if xb_dev.dtype != self._xb.dtype or xb_dev.dim() != 2 or xb_dev.shape[1] != self.dim or not xb_dev.is_contiguous():
            raise ValueError("adopt() needs a contiguous device matrix [n, rr_padded_dim(d)] of the index dtype")
        self._xb = xb_dev
        self.ntotal = int(xb_dev.shape[0] if ntotal is None else ntotal)
        self._x8 = self._x8_stats = None
        self._refresh_norms()

    def build_screen(self, list_len=None):
        """Build the int8 screening copy of the current corpus (+50 % HBM).  list_len: rows per query that are re-scored
        exactly (k <= list_len <= 1024; default max(512, 16 k) capped at 1024)."""
        if self.metric == "l2":
            raise _lib.RagrouteHipError("the int8 screening copy serves the ip / cosine metrics only")
        if self.exact_f32:
            raise _lib.RagrouteHipError("the int8 screening copy and exact_f32 do not combine")
        dim8 = lib().rr_screen_dim(self.dim)
        if dim8 < 0:
            raise _lib.RagrouteHipError("the int8 screening copy needs d <= 1536")
        if list_len is not None:
            self.screen_list = int(list_len)
        self._x8 = torch.empty((max(1, self.ntotal), dim8), dtype=torch.int8, device=self.device)
        self._x8_stats = torch.zeros(8, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().rr_screen_build(self._xb.data_ptr(), _calls.RR_DTYPE[self.dtype], self.ntotal, self.dim, self._x8.data_ptr(),
                                        self._x8_stats.data_ptr(), _calls.stream_ptr()), "rr_screen_build")
        return self

    def search_screened(self, xq_half, k, id_offset=0, out=None, route_mask=None, list_len=None):
        """Device-to-device search through the int8 screening copy: (D, I, exact) CUDA tensors; exact[q] == 1 where the result
        is proven to be the exact top-k.  No host sync; search_prepared() wraps this with the check and the fallback."""
        if self._x8 is None:
            raise _lib.RagrouteHipError("build_screen() has not been called (or the corpus changed since)")
        nq = xq_half.shape[0]
        L = int(list_len if list_len is not None else min(_lib.RR_MAX_K, max(self.screen_list, 16 * k)))
        L = max(L, k)
        ws = _calls.workspace(self._ws_screen, (k, L, nq), self.device, _LIST_RANGE, "rr_flat_search_screened_workspace_bytes",
                              k, L, nq, self.dim)
        D, I = _calls.out_pair(nq, k, self.device, out)
        exact = torch.empty(nq, dtype=torch.uint8, device=self.device)
        mptr, mstride = self._mask_args(route_mask, nq)
        check(lib().rr_flat_search_screened(self._xb.data_ptr(), _calls.RR_DTYPE[self.dtype], self._x8.data_ptr(), self._x8_stats.data_ptr(),
                                            self.ntotal, self.dim, xq_half.data_ptr(), nq, k, L, D.data_ptr(), I.data_ptr(), id_offset,
                                            exact.data_ptr(), ws.data_ptr(), ws.numel(), mptr, mstride, _calls.stream_ptr()),
              "rr_flat_search_screened")
        return D, I, exact

    def centroid(self):
        """float32 CUDA vector [d]: mean of the stored rows (the router's centroid feature, router.py:147-151)."""
        out = torch.empty(self.dim, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().rr_centroid(self._xb.data_ptr(), _calls.RR_DTYPE[self.dtype], self.ntotal, self.dim, self.d, out.data_ptr(),
                                    _calls.stream_ptr()), "rr_centroid")
        return out[: self.d]

    @property
    def xb(self):
        return self._xb[: self.ntotal]

    # -- search ------------------------------------------------------------------------------
    def search_prepared(self, xq_half, k, id_offset=0, out=None, route_mask=None):
        """Device-to-device search: xq_half [nq,dim] index dtype -> (D f32[nq,k], I i64[nq,k]) CUDA tensors.
        route_mask: optional bool/uint8 CUDA tensor [nq] (may be a strided column of the router's [nq,C] mask):
        queries with a zero entry get an all-padding result.  Enqueued on the current stream, no host sync.
        exact_f32 / exact_l2: xq_half is the (half, f32) pair of prepare_queries(); one host read of the proof flags."""
        if self._faith:
            return self._faithful_search(xq_half, k, route_mask, out, self._segments(id_offset, route_mask), self.ntotal)
        _calls.check_half_queries(xq_half, self._xb.dtype, self.dim, "search_prepared() needs contiguous [nq, dim] queries of the index dtype")
        if self._x8 is not None and xq_half.shape[0] > 0:
            # screened search; the proof flags are the one host read of this path
            D, I, exact = self.search_screened(xq_half, k, id_offset, out, route_mask)
            if bool(exact.all()):
                return D, I
            self.screen_fallbacks += 1
            out = (D, I)
        return self._half_search(xq_half, k, route_mask, out, self.ntotal, id_offset)

    def search(self, xq, k):
        """faiss call shape: float32 [nq,d] -> (D float32[nq,k], I int64[nq,k]) numpy arrays."""
        return super().search(xq, k)


class SegmentedIndex(_Index):
    """Several data sources that are searched with the SAME query embeddings, resident in ONE HBM matrix and searched in ONE
    pass (C ABI `rr_flat_search_segments`): MedRAG's four sources all use MedCPT, five FeB4RAG sources UAE-Large-V1
    (reference ragroute/config.py:37-71).  The reference asks every selected source separately (`index.search`,
    data_source.py:158, 186, 203) and its front-end concatenates the replies and keeps the k best (http_server.py:280-293,
    rerank.py:3-9); `search_prepared` returns exactly that merged list — per query, the k best rows of the union of the
    sources the router selected for it — with one query preparation, one bootstrap and one chunk schedule for all of them.

    Source s occupies rows [begin_s, begin_s + n_s) of the matrix, begin_s a multiple of 256; `source(s)` is a FlatIndex on that
    slice (no copy), so the per-source call surface (`DataSource.retrieve_docs_*`) keeps working on the same memory.
    Result ids are id_offsets[s] + local row; ties are broken by (source order, row) = ascending id when the id offsets ascend.
    Metrics: "ip" / "cosine", and "l2" (C ABI `rr_flat_search_segments_l2`: squared L2 distances, nearest first, padding
    (+inf, -1) — the reference's wikipedia federation, ten sources of one DPR encoder whose merge keeps the lowest scores,
    config.py:59-70, rerank.py:28-34); `_hn` then holds |x|^2 / 2 of every matrix row, filled source by source.
    exact_f32=True (ip / cosine), exact_l2=True (l2): f32 rows beside the half matrix, results faithful to them (FlatIndex)."""

    def __init__(self, d, rows_per_source, id_offsets=None, mask_cols=None, metric="ip", dtype="fp16", device=None, exact_f32=False,
                 exact_l2=False):
        rows = [int(n) for n in rows_per_source]
        if not 1 <= len(rows) <= _lib.RR_MAX_SEGMENTS or min(rows) < 0:
            raise ValueError(f"need 1 .. {_lib.RR_MAX_SEGMENTS} sources with >= 0 rows each")
        super().__init__(d, metric, dtype, device, exact_f32, exact_l2)
        self.rows = rows
        self.id_offsets = [int(v) for v in (id_offsets if id_offsets is not None else [s << 40 for s in range(len(rows))])]
        self.mask_cols = [int(v) for v in (mask_cols if mask_cols is not None else range(len(rows)))]
        if len(self.id_offsets) != len(rows) or len(self.mask_cols) != len(rows):
            raise ValueError("one id offset and one mask column per source")
        A = _lib.RR_SEGMENT_ALIGN
        self.begins, off = [], 0
        for n in rows:
            self.begins.append(off)
            off += -(-n // A) * A
        self.n_rows_total = self.begins[-1] + rows[-1]            # nothing behind the last valid row is ever read
        if self.n_rows_total > 0xFFFFFFE0:
            raise ValueError("more than 2^32 - 32 rows in one segmented matrix")
        self._xb = torch.zeros((max(1, self.n_rows_total), self.dim), dtype=_calls.TORCH_DTYPE[dtype], device=self.device)
        self._segs = (_lib.SegmentStruct * len(rows))(*[_lib.SegmentStruct(b, n, o, c, 0)
                                                        for b, n, o, c in zip(self.begins, rows, self.id_offsets, self.mask_cols)])
        self.ntotal = sum(rows)
        if metric == "l2":   # aligned with _xb (alignment gaps: unspecified, never used)
            self._hn = torch.zeros(max(1, self.n_rows_total), dtype=torch.float32, device=self.device)
        self._faithful_init(self.n_rows_total)

    @property
    def _n_rows(self):
        return self.n_rows_total

    def _segments(self, id_offset=0, route_mask=None):
        return self._segs

    def _mask_args(self, route_mask, nq):
        if route_mask is None:
            return None, 0
        if (route_mask.dtype not in (torch.bool, torch.uint8) or route_mask.dim() != 2 or route_mask.shape[0] != nq
                or not route_mask.is_cuda or route_mask.stride(1) != 1 or route_mask.shape[1] <= max(self.mask_cols)):
            raise ValueError("route_mask must be a bool/uint8 CUDA matrix [nq, C] with unit column stride covering every mask column")
        return route_mask.data_ptr(), route_mask.stride(0)

    # -- storage -----------------------------------------------------------------------------
    def rows_of(self, s):
        """Device view [n_s, dim] of source s (fill it with rows in the index dtype, zero padded to dim)."""
        return self._xb[self.begins[s]: self.begins[s] + self.rows[s]]

    def norms_of(self, s):
        """Metric "l2": device view [n_s] of source s's half squared norms."""
        return self._hn[self.begins[s]: self.begins[s] + self.rows[s]]

    def refresh_norms(self, s):
        """Metric "l2": recompute source s's half squared norms from its stored rows (fill() does; call it after writing
        rows_of(s) directly)."""
        if self.metric != "l2" or self.rows[s] == 0:
            return
        with torch.cuda.device(self.device):
            _calls.half_sqnorms(self.rows_of(s), self.rows[s], self.norms_of(s))

    def _point_at(self, idx, s):
        """Make FlatIndex idx a view of source s: its rows and, for "l2", its slice of the norms (nothing is recomputed)."""
        idx._xb, idx.ntotal = self.rows_of(s), self.rows[s]
        idx._x8 = idx._x8_stats = None
        idx._hn = self.norms_of(s) if self.metric == "l2" and self.rows[s] else None
        return idx

    def source(self, s):
        """FlatIndex over source s's slice of the matrix (no copy): the per-source search surface on the same memory."""
        return self._point_at(FlatIndex(self.d, metric=self.metric, dtype=self.dtype, device=self.device), s)

    def fill(self, s, x, chunk_rows=1 << 18):
        """Ingest float32 rows [n_s, d] (numpy or tensor) into source s (normalised for cosine)."""
        if x.shape[0] != self.rows[s] or x.shape[1] != self.d:
            raise ValueError(f"source {s} holds [{self.rows[s]}, {self.d}] rows")
        with torch.cuda.device(self.device):
            self._ingest(x, self.begins[s], chunk_rows)
            self._faithful_build()
        self.refresh_norms(s)

    @classmethod
    def from_indexes(cls, indexes, id_offsets=None, mask_cols=None):
        """Pack existing FlatIndex objects (same d / metric / dtype / device) into one matrix and re-point each of them at its
        slice, so their own buffers can be released."""
        first = indexes[0]
        for i in indexes:
            if (i.d, i.metric, i.dtype, i.device) != (first.d, first.metric, first.dtype, first.device):
                raise ValueError("sources of one SegmentedIndex share dimension, metric, dtype and device")
        seg = cls(first.d, [i.ntotal for i in indexes], id_offsets, mask_cols, first.metric, first.dtype, first.device)
        for s, i in enumerate(indexes):
            if i._faith:
                raise _lib.RagrouteHipError("from_indexes() packs half matrices only; an exact_f32 / exact_l2 index ingests its f32 rows with fill()")
            seg.rows_of(s).copy_(i.xb)
            if first.metric == "l2" and i.ntotal:
                seg.norms_of(s).copy_(i._hn[: i.ntotal])
            seg._point_at(i, s)
        return seg

    # -- search ------------------------------------------------------------------------------
    def search_prepared(self, xq_half, k, route_mask=None, out=None):
        """xq_half [nq, dim] index dtype -> (D f32 [nq,k], I i64 [nq,k]) CUDA tensors: the merged top-k over the selected sources.
        route_mask: optional bool/uint8 CUDA matrix [nq, C] (the router's mask; source s reads column mask_cols[s]).
        exact_f32 / exact_l2: xq_half is the (half, f32) pair of prepare_queries()."""
        if self._faith:
            return self._faithful_search(xq_half, k, route_mask, out, self._segs, self.n_rows_total)
        _calls.check_half_queries(xq_half, self._xb.dtype, self.dim, "search_prepared() needs contiguous [nq, dim] queries of the index dtype")
        return self._half_search(xq_half, k, route_mask, out, self.n_rows_total, segs=self._segs)

    def search_exact_f32(self, xq_f32_dev, k, list_len=None, route_mask=None):
        """As FlatIndex.search_exact_f32, over the segments (route_mask [nq, C] as search_prepared)."""
        return super().search_exact_f32(xq_f32_dev, k, list_len, route_mask)
