"""Cost of the f32-faithful mode (FlatIndex exact_f32=True, or exact_l2=True with --metric l2) against the plain search of the
same half rows: one JSON line per shape.

    PYTHONPATH=. python tools/faithful_perf.py [--metric ip|l2] [--shapes iid,clustered,wide,l2_1m] [--iters 10] [--out FILE]

Per shape: ms per batch of the plain search and of the faithful one (search_prepared: proof, retry, fallback, one host read),
the split of the faithful device work into the scan at k' = list_len (the plain segmented search at that k), the re-score (the
rest of search_exact_f32) and what the retry / fallback add, the proven fraction at the default list_len, and the retry and
fallback counts of one batch, and the exact f32 scan's ms per query (one launch of 16 queries).  Rows are generated on the device
(i.i.d. gaussian, or gaussian around 1000 centres)."""
import argparse
import json
import sys

import torch

from ragroute_amd._calls import half_search
from ragroute_amd.flat_index import FlatIndex

SHAPES = {  # name: rows, d, queries, k, corpus
    "iid": (10_000_000, 768, 256, 32, "iid"),
    "clustered": (10_000_000, 768, 256, 32, "clustered"),
    "wide": (2_000_000, 2048, 256, 100, "iid"),
    "l2_1m": (1_000_000, 768, 256, 32, "iid"),
}


def rows(gen, n, d, kind, centres, dev):
    t = torch.randn((n, d), generator=gen, device=dev)
    if kind == "clustered":
        t = centres[torch.randint(0, centres.shape[0], (n,), generator=gen, device=dev)] + t * (0.3 / d ** 0.5)
    return t


def timed(f, iters):
    f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def measure(name, iters, metric="ip"):
    n, d, nq, k, kind = SHAPES[name]
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    centres = torch.randn((1000, d), generator=gen, device=dev) / d ** 0.5 if kind == "clustered" else None
    l2 = metric == "l2"
    idx = FlatIndex(d, metric=metric, device=dev, **({"exact_l2": True} if l2 else {"exact_f32": True}))
    idx.reserve(n)
    chunk = 1 << 20
    for s in range(0, n, chunk):
        idx.add(rows(gen, min(chunk, n - s), d, kind, centres, dev))
    xq = rows(gen, nq, d, kind, centres, dev)
    plain = FlatIndex(d, metric=metric, device=dev)
    plain.adopt(idx.xb)
    prep = idx.prepare_queries(xq)
    L = idx._faithful_list_len(k)
    seg = idx._segments()
    # the scan of the faithful search alone: the same segmented scan at k' = list_len (rr_flat_search_segments / _segments_l2)
    ws = plain._workspace(L)
    DL = torch.empty((nq, L), dtype=torch.float32, device=dev)
    IL = torch.empty((nq, L), dtype=torch.int64, device=dev)

    def scan_only():
        half_search(idx._xb, idx.ntotal, prep[0], L, DL, IL, ws, None, 0, segs=seg, l2=l2, hn=idx._hn)
    t_plain = timed(lambda: plain.search_prepared(prep[0], k), iters)
    t_scan = timed(scan_only, iters)
    t_raw = timed(lambda: idx._faithful_raw(prep[0], prep[1], k, L, seg, idx.ntotal, None, 0), iters)
    _, _, exact, eps = idx._faithful_raw(prep[0], prep[1], k, L, seg, idx.ntotal, None, 0)
    proven = float(exact.float().mean())
    r0, f0 = idx.faithful_retries, idx.faithful_fallbacks
    idx.search_prepared(prep, k)
    retries, fallbacks = idx.faithful_retries - r0, idx.faithful_fallbacks - f0
    t_full = timed(lambda: idx.search_prepared(prep, k), iters)
    nx = min(16, nq)   # one launch of the exact scan
    Dx = torch.empty((nq, k), dtype=torch.float32, device=dev)
    Ix = torch.empty((nq, k), dtype=torch.int64, device=dev)
    qx = torch.arange(nx, dtype=torch.int32, device=dev)
    t_exact = timed(lambda: idx._exact_scan(prep[1], qx, k, seg, idx.ntotal, None, 0, Dx, Ix), iters)
    return {"shape": name, "metric": metric, "rows": n, "d": d, "queries": nq, "k": k, "corpus": kind, "list_len": L, "dtype": "fp16",
            "plain_ms": round(t_plain, 4), "faithful_ms": round(t_full, 4), "ratio": round(t_full / t_plain, 3),
            "split_ms": {"scan_at_list_len": round(t_scan, 4), "rescore": round(t_raw - t_scan, 4),
                         "retry_fallback_and_host_read": round(t_full - t_raw, 4)},
            "proven_fraction": proven, "retries_per_batch": retries, "fallbacks_per_batch": fallbacks,
            "exact_scan_ms_per_query": round(t_exact / nx, 4),
            **({"A_median": float(eps[:, 0].median()), "R_median": float(eps[:, 1].median())} if l2 else {"eps_median": float(eps.median())}),
            "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--metric", default="ip", choices=["ip", "l2"])
    ap.add_argument("--shapes", default=None, help="default: iid,clustered,wide (ip), l2_1m (l2)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None
    for name in (a.shapes or ("l2_1m" if a.metric == "l2" else "iid,clustered,wide")).split(","):
        line = json.dumps(measure(name, a.iters, a.metric))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
