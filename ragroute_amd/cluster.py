"""Cluster one corpus into a routed federation (k-means on the GPU).

The reference's wikipedia federation is one DPR index cut into ten k-means clusters (`NUM_CLUSTERS = 10`,
scripts/train/train_mmlu_router.py:26-30; `faiss_index_{c}_normalized.index`, ragroute/data_source.py:55-62; sources named by
cluster number, ragroute/router.py:140-144).  It only consumes those files; this module makes them:

    kmeans(index, C)             Lloyd iterations over the stored rows of a FlatIndex        -> Clustering
    federate(index, clustering)  the clusters as the sources of ONE SegmentedIndex           -> Federation
    route_nearest(clustering, xq, n_probe)   the router a fresh federation has before anyone trains an MLP: a route mask
    cluster_stats / write_federation         the `cluster_stats.json` list and the on-disk layout DataSource("wikipedia") loads

All arithmetic is in libragroute_hip.so (rr_cluster_assign, rr_cluster_means, rr_rows_to_half, rr_half_sqnorms,
rr_l2_normalize_f32, the flat search); PyTorch is memory, a stable sort, gathers, comparisons and the counting of labels.
"""
import json
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _calls
from . import _lib
from ._lib import check, lib
from .flat_index import FlatIndex, SegmentedIndex

_ID_SHIFT = 40   # federation ids are (cluster << 40) + row inside the cluster, as SegmentedIndex numbers its sources


class Clustering(NamedTuple):
    centroids: torch.Tensor   # f32 [C, d] on the index's device (unit rows for the spherical metrics)
    assign: torch.Tensor      # i32 [n]: the assignment against `centroids` (-1: a row whose every score is NaN)
    counts: torch.Tensor      # i64 [C]: members per cluster under `assign`
    iterations: int           # passes of the [assign, means] loop that ran
    converged: bool           # a pass changed no label
    metric: str = "l2"
    dtype: str = "fp16"


def _plain(index):
    if not isinstance(index, FlatIndex):
        raise ValueError("clustering takes a plain FlatIndex")
    if index._faith or index._x8 is not None:
        raise _lib.RagrouteHipError("clustering an exact_f32 / exact_l2 or screened index is not supported: cluster a plain FlatIndex")
    return index


def _half_centroids(index, centroids):
    """f32 [C, d] -> ([C, dim] in the index dtype, NOT normalised; the L2 bias |c|^2 / 2 of those half rows, or None)."""
    c = _calls.f32_queries(centroids, index.d, index.device)
    if not 1 <= c.shape[0] <= _lib.RR_MAX_CLUSTERS:
        raise ValueError(f"need 1 .. {_lib.RR_MAX_CLUSTERS} centroids, got {c.shape[0]}")
    ch = _calls.rows_to_half(c, index.dim, index._xb.dtype, False)
    return ch, (_calls.half_sqnorms(ch, ch.shape[0]) if index.metric == "l2" else None)


def assign_half(xb, n_rows, cent_half, bias, out=None):
    """rr_cluster_assign on n_rows rows of the half matrix xb against the half centroids: (assign i32 [n], score f32 [n])."""
    a, s = out if out is not None else (torch.empty(n_rows, dtype=torch.int32, device=xb.device),
                                        torch.empty(n_rows, dtype=torch.float32, device=xb.device))
    check(lib().rr_cluster_assign(xb.data_ptr(), _calls.dtype_code(xb), n_rows, xb.shape[1], cent_half.data_ptr(),
                                  bias.data_ptr() if bias is not None else None, cent_half.shape[0], a.data_ptr(), s.data_ptr(),
                                  _calls.stream_ptr()), "rr_cluster_assign")
    return a, s


def assign(index, centroids):
    """Nearest centroid of every stored row: (assign i32 [n], score f32 [n]) on the device.  centroids f32 [C, d] are rounded to the
    index dtype without normalisation; "l2" scores x . c - |c|^2 / 2 (nearest under squared L2), "ip" / "cosine" score x . c."""
    _plain(index)
    with torch.cuda.device(index.device):
        ch, bias = _half_centroids(index, centroids)
        return assign_half(index._xb, index.ntotal, ch, bias)


def means(index, labels, centroids, ws=None):
    """rr_cluster_means: row c of `centroids` (f32 [C, d], in place) becomes the mean of the stored rows labelled c; returns the
    counts i64 [C].  A cluster without members keeps its row."""
    C = centroids.shape[0]
    if ws is None:
        ws = _calls.workspace({}, 0, index.device, "bad clustering sizes: n_rows={0}, dim={1}, n_clusters={2}", "rr_cluster_workspace_bytes",
                              index.ntotal, index.dim, C)
    counts = torch.empty(C, dtype=torch.int64, device=index.device)
    check(lib().rr_cluster_means(index._xb.data_ptr(), _calls.RR_DTYPE[index.dtype], index.ntotal, index.dim, index.d, labels.data_ptr(), C,
                                 centroids.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), _calls.stream_ptr()), "rr_cluster_means")
    return counts


def kmeans(index, n_clusters, iters=20, seed=0, init=None):
    """Lloyd's k-means over the stored rows of a plain FlatIndex.  The metric comes from the index: "l2" is Euclidean; "ip" and
    "cosine" are spherical (centroids normalised by rr_l2_normalize_f32 after every update, assignment by inner product).
    init: f32 [C, d], or the stored rows at sorted(numpy.random.default_rng(seed).choice(n, C, replace=False)).
    The loop is [assign, stop if no label changed, means] up to `iters` times (one host read per pass: the changed count), then one
    final assign, so `assign` is always the assignment against the returned `centroids`.  An empty cluster keeps its centroid."""
    _plain(index)
    C, n = int(n_clusters), index.ntotal
    if not 1 <= C <= _lib.RR_MAX_CLUSTERS:
        raise ValueError(f"n_clusters must be in [1, {_lib.RR_MAX_CLUSTERS}], got {C}")
    if n < C:
        raise ValueError(f"{n} rows cannot make {C} clusters")
    with torch.cuda.device(index.device):
        if init is None:
            rows = sorted(int(r) for r in np.random.default_rng(seed).choice(n, C, replace=False))
            cent = index._xb[torch.tensor(rows, device=index.device)][:, : index.d].to(torch.float32).contiguous()
        else:
            cent = _calls.f32_queries(init, index.d, index.device).clone()
            if cent.shape[0] != C:
                raise ValueError(f"init must be [{C}, {index.d}]")
        spherical = index.metric != "l2"
        ws = _calls.workspace({}, 0, index.device, "bad clustering sizes: n_rows={0}, dim={1}, n_clusters={2}", "rr_cluster_workspace_bytes",
                              n, index.dim, C)
        prev = torch.full((n,), -2, dtype=torch.int32, device=index.device)
        iterations, converged = 0, False
        for _ in range(int(iters)):
            ch, bias = _half_centroids(index, cent)
            cur, _score = assign_half(index._xb, n, ch, bias)
            iterations += 1
            if int((cur != prev).sum()) == 0:     # the pass's one host read
                converged = True
                break
            prev = cur
            means(index, cur, cent, ws)
            if spherical:
                _calls.l2_normalize_(cent)
        ch, bias = _half_centroids(index, cent)
        final, _score = assign_half(index._xb, n, ch, bias)
        counts = torch.bincount(final[final >= 0].to(torch.int64), minlength=C)
    return Clustering(cent, final, counts, iterations, converged, index.metric, index.dtype)


class Federation:
    """The clusters of one corpus as the sources of a SegmentedIndex: `index` (search it with search_prepared(route_mask=...)),
    `rows` i64 [n_kept] = the original row of every federation row (cluster by cluster, ascending inside a cluster), `starts` i64
    [C + 1] = where each cluster begins in `rows`."""

    def __init__(self, index, rows, starts):
        self.index, self.rows, self.starts = index, rows, starts

    def original_ids(self, I):
        """Result ids of the federation ((cluster << 40) + row inside the cluster) -> original rows; -1 stays -1."""
        keep = I >= 0
        safe = torch.where(keep, I, torch.zeros_like(I))
        pos = self.starts[safe >> _ID_SHIFT] + (safe & ((1 << _ID_SHIFT) - 1))
        return torch.where(keep, self.rows[pos], torch.full_like(I, -1))


def federate(index, clustering, drop_unassigned=False):
    """A SegmentedIndex of the index's metric and dtype whose source c holds the stored half rows of cluster c, in ascending original
    row order, copied bit for bit (norms refreshed for "l2"); id offsets c << 40, mask columns c.  Rows labelled -1 raise unless
    drop_unassigned.  (A SegmentedIndex holds at most RR_MAX_SEGMENTS = 32 sources.)"""
    _plain(index)
    labels = clustering.assign
    C = clustering.centroids.shape[0]
    if labels.shape[0] != index.ntotal:
        raise ValueError("the clustering does not belong to this index")
    with torch.cuda.device(index.device):
        order = torch.sort(labels, stable=True).indices       # cluster by cluster, ascending row inside each; -1 first
        n_drop = int((labels < 0).sum())
        if n_drop and not drop_unassigned:
            raise ValueError(f"{n_drop} rows are assigned to no cluster (NaN scores); pass drop_unassigned=True to leave them out")
        rows = order[n_drop:].contiguous()
        sizes = torch.bincount(labels[rows].to(torch.int64), minlength=C).cpu().tolist()
        seg = SegmentedIndex(index.d, sizes, metric=index.metric, dtype=index.dtype, device=index.device)
        starts = [0]
        for c, m in enumerate(sizes):
            if m:
                torch.index_select(index._xb, 0, rows[starts[-1]: starts[-1] + m], out=seg.rows_of(c))
                seg.refresh_norms(c)
            starts.append(starts[-1] + m)
    return Federation(seg, rows, torch.tensor(starts, dtype=torch.int64, device=index.device))


def centroid_index(clustering):
    """A FlatIndex over the C centroids, rounded exactly as assign() rounds them (no normalisation)."""
    idx = FlatIndex(clustering.centroids.shape[1], metric=clustering.metric, dtype=clustering.dtype, device=clustering.centroids.device)
    with torch.cuda.device(idx.device):
        idx.adopt(_calls.rows_to_half(clustering.centroids.contiguous(), idx.dim, idx._xb.dtype, False))
    return idx


def route_nearest(clustering_or_centroid_index, xq, n_probe):
    """u8 mask [nq, C]: the n_probe best clusters of every query by the score assignment uses - the existing flat search over the C
    centroids plus a scatter.  Pass it as route_mask= to the federation's SegmentedIndex.search_prepared."""
    idx = clustering_or_centroid_index
    if isinstance(idx, Clustering):
        idx = centroid_index(idx)
    C = idx.ntotal
    if not 1 <= int(n_probe) <= C:
        raise ValueError(f"n_probe must be in [1, {C}], got {n_probe}")
    with torch.cuda.device(idx.device):
        _D, I = idx.search_prepared(idx.prepare_queries(xq), int(n_probe))
        mask = torch.zeros((I.shape[0], C), dtype=torch.uint8, device=idx.device)
        mask.scatter_(1, torch.where(I >= 0, I, torch.zeros_like(I)), (I >= 0).to(torch.uint8))   # a NaN query selects nothing
    return mask


def cluster_stats(index, clustering):
    """[{"centroid": [d floats], "size": int}] indexed by cluster - what Router.load_router reads for wikipedia
    (`cluster_stats.json`).  The centroid is the mean of the final members (one rr_cluster_means call), not the spherical one."""
    _plain(index)
    with torch.cuda.device(index.device):
        cent = torch.zeros_like(clustering.centroids, dtype=torch.float32).contiguous()
        counts = means(index, clustering.assign, cent)
        cent, counts = cent.cpu().numpy(), counts.cpu().tolist()
    return [{"centroid": [float(v) for v in cent[c]], "size": int(counts[c])} for c in range(len(counts))]


def write_federation(root, x_f32, assign, stats, titles=None, texts=None, metric="l2"):
    """Host only: write the layout DataSource("wikipedia") and the router load under `root` (the wikipedia dataset directory):
        faiss_clusters/normalized_indexes/faiss_index_{c}_normalized.index     cluster c's f32 rows, ascending original row
        faiss_clusters/split_texts_titles/{titles,texts}_{c}.txt               one line per row (empty lines without titles / texts)
        faiss_clusters/cluster_stats.json                                      `stats` (cluster_stats())
    x_f32 [n, d] numpy / memmap, assign [n] integers (rows outside [0, len(stats)) are left out)."""
    from .data_source import write_faiss_flat_index
    assign = np.asarray(assign).astype(np.int64)
    if assign.shape != (x_f32.shape[0],):
        raise ValueError("one label per row")
    for lines in (titles, texts):
        if lines is not None and len(lines) != x_f32.shape[0]:
            raise ValueError("one title and one text per row")
    base = os.path.join(root, "faiss_clusters")
    os.makedirs(os.path.join(base, "normalized_indexes"), exist_ok=True)
    os.makedirs(os.path.join(base, "split_texts_titles"), exist_ok=True)
    for c in range(len(stats)):
        rows = np.flatnonzero(assign == c)
        write_faiss_flat_index(os.path.join(base, "normalized_indexes", f"faiss_index_{c}_normalized.index"),
                               np.asarray(x_f32[rows], np.float32).reshape(len(rows), x_f32.shape[1]), metric="l2" if metric == "l2" else "ip")
        for name, lines in (("titles", titles), ("texts", texts)):
            with open(os.path.join(base, "split_texts_titles", f"{name}_{c}.txt"), "w", encoding="utf-8") as f:
                f.write("".join((lines[r] if lines is not None else "") + "\n" for r in rows))
    with open(os.path.join(base, "cluster_stats.json"), "w") as f:
        json.dump(stats, f)
