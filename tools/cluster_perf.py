"""Cost of clustering a stored corpus: one assignment pass (rr_cluster_assign), one means pass (rr_cluster_means) and a full
10-iteration kmeans on rows x d fp16 rows with C = 10 and C = 64 - and, in the same process on the same device, one plain
rr_flat_search of C queries, k = 1, over the same rows: code that streams the same bytes and exists without the clustering
kernels.  It is the yardstick.  Times are HIP events around `reps` back-to-back calls after a warm-up; bytes/s counts the corpus
bytes once per pass (the centroids and outputs are three orders of magnitude smaller).

    python tools/cluster_perf.py [--rows 10000000] [--d 768] [--clusters 10,64] [--reps 5] [--out profiles/cluster/cluster_perf.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragroute_amd import cluster  # noqa: E402
from ragroute_amd.flat_index import FlatIndex  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--clusters", default="10,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--metric", default="l2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cluster_perf.py needs a HIP device"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    idx = FlatIndex(args.d, args.metric, "fp16", device=dev)
    n = args.rows
    xb = torch.zeros((n, idx.dim), dtype=torch.float16, device=dev)
    n_blobs = 64                                       # loosely clustered data, so that kmeans has labels to move
    centres = torch.randn((n_blobs, args.d), generator=g, device=dev) / args.d ** 0.5
    for s in range(0, n, 1 << 20):
        e = min(n, s + (1 << 20))
        which = torch.randint(0, n_blobs, (e - s,), generator=g, device=dev)
        xb[s:e, : args.d] = (centres[which] + torch.randn((e - s, args.d), generator=g, device=dev) / args.d ** 0.5).half()
    idx.adopt(xb)
    corpus_bytes = n * idx.dim * 2
    lines = []
    for C in [int(c) for c in args.clusters.split(",")]:
        init = xb[torch.randperm(n, generator=g, device=dev)[:C]][:, : args.d].float()
        ch, bias = cluster._half_centroids(idx, init)
        labels, _ = cluster.assign_half(xb, n, ch, bias)
        out = (labels, torch.empty(n, dtype=torch.float32, device=dev))
        cent = init.clone()
        ws = torch.empty(cluster.lib().rr_cluster_workspace_bytes(n, idx.dim, C), dtype=torch.uint8, device=dev)
        xq = idx.prepare_queries(init)
        assign_ms = timed(lambda: cluster.assign_half(xb, n, ch, bias, out), args.reps)
        means_ms = timed(lambda: cluster.means(idx, labels, cent, ws), args.reps)
        search_ms = timed(lambda: idx.search_prepared(xq, 1), args.reps)
        result = {}

        def run_kmeans():
            result["r"] = cluster.kmeans(idx, C, iters=10, init=init)
        kmeans_ms = timed(run_kmeans, 1)
        r = result["r"]
        line = {"rows": n, "d": args.d, "dim": idx.dim, "dtype": "fp16", "metric": args.metric, "clusters": C, "reps": args.reps,
                "assign_ms": round(assign_ms, 3), "assign_TBps": round(corpus_bytes / assign_ms / 1e9, 3),
                "means_ms": round(means_ms, 3), "means_TBps": round(corpus_bytes / means_ms / 1e9, 3),
                "flat_search_C_queries_k1_ms": round(search_ms, 3), "flat_search_TBps": round(corpus_bytes / search_ms / 1e9, 3),
                "assign_over_search": round(assign_ms / search_ms, 3), "means_over_search": round(means_ms / search_ms, 3),
                "kmeans_10_iterations_ms": round(kmeans_ms, 1), "kmeans_passes": r.iterations, "kmeans_converged": r.converged,
                "workspace_MiB": round(ws.numel() / 2 ** 20, 1), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
