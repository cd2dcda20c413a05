"""Cost of the one-pass segmented squared-L2 search (rr_flat_search_segments_l2) against what the library could do for the same
inputs before it existed: one rr_flat_search_l2 per source + the ascending merge of the per-source lists.

    python tools/segments_l2_perf.py --baseline-lib OLD.so [--lib NEW.so] [--searches 50] [--alternations 3] [--out DIR] [--scale F]

OLD.so is a libragroute_hip.so built from the commit before the segmented L2 search (it has no rr_flat_search_segments_l2); NEW.so
defaults to the tree's library.  Each library is loaded by a child process of its own (plain ctypes, nothing of the package: the
package's binding declares symbols the old library lacks).  Both children build the SAME seeded federation in the same matrix layout
(sources at multiples of 256 rows), the parent checks that both return identical ids and distances for the timed queries, and
then alternates timed legs between them - device events over `--searches` back-to-back searches per leg after a warm-up,
`--alternations` rounds - so that both versions see the same machine state.  Recorded per federation: every leg, the baseline's
run-to-run spread (max - min of its legs), and for information the segmented inner-product search of the same matrix (no norm
stream) and the plain L2 / IP searches of the whole matrix as one corpus (the L2 / IP ratio of a plain search on the same device).

Workloads (256 queries, k = 10, fp16):
  wikipedia  ten L2 sources of 2.1 M x 768 rows: the DPR Wikipedia dump's 21 M passages in ten parts.  The reference names ten
             wikipedia clusters behind one DPR question encoder (config.py:35, 59-70) but states no per-cluster counts: the equal
             split is an ASSUMPTION of this tool.
  uae        FeB4RAG's five UAE-Large-V1 sources (nfcorpus, arguana, dbpedia-entity, fever, climate-fever; public BEIR counts)
             at d = 1024, stored as L2.
Baseline merge: rr_merge_topk_gathered over the per-source lists where they lie (the same kernel as rr_merge_topk, without the
copy that would bring the lists into its [nq][S k] layout: the cheapest form the old library offers)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, K, ALIGN, SHIFT = 256, 10, 256, 40
FEDERATIONS = {
    "wikipedia": {"dim": 768, "rows": [2_100_000] * 10,
                  "note": "ten equal parts of the DPR Wikipedia dump's 21 M passages: per-cluster counts are an assumption (the reference states none)"},
    "uae": {"dim": 1024, "rows": [3_633, 8_674, 4_635_922, 5_416_568, 5_416_593],
            "note": "FeB4RAG's five UAE-Large-V1 sources (public BEIR document counts), stored as L2"},
}


class Segment(ctypes.Structure):      # struct rr_segment
    _fields_ = [("row_begin", ctypes.c_int64), ("n_rows", ctypes.c_int64), ("id_offset", ctypes.c_int64), ("mask_col", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


def load(path):
    L = ctypes.CDLL(path)
    vp, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    L.rr_last_error.restype = ctypes.c_char_p
    L.rr_flat_search_workspace_bytes_for.argtypes = [i32, i32]
    L.rr_flat_search_workspace_bytes_for.restype = sz
    L.rr_half_sqnorms.argtypes = [vp, i32, i64, i32, vp, vp]
    L.rr_flat_search.argtypes = [vp, i32, i64, i32, vp, i32, i32, vp, vp, i64, vp, sz, vp, i64, vp]
    L.rr_flat_search_l2.argtypes = [vp, vp, i32, i64, i32, vp, i32, i32, vp, vp, i64, vp, sz, vp, i64, vp]
    L.rr_flat_search_segments.argtypes = [vp, i32, i64, i32, ctypes.POINTER(Segment), i32, vp, i32, i32, vp, vp, vp, sz, vp, i64, vp]
    L.rr_merge_topk_gathered.argtypes = [vp, i32, sz, sz, i32, i32, i32, i32, i32, vp, vp, vp]
    if hasattr(L, "rr_flat_search_segments_l2"):
        L.rr_flat_search_segments_l2.argtypes = [vp, vp, i32, i64, i32, ctypes.POINTER(Segment), i32, vp, i32, i32, vp, vp, vp, sz, vp, i64, vp]
    return L


# ---- child: one library, commands as JSON lines on stdin, one JSON line of answer each --------------------------------------------
def worker(lib_path):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("segments_l2_perf: no HIP device")
    L = load(lib_path)
    dev = torch.device("cuda:0")
    st = {}

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: status {rc}: {L.rr_last_error().decode()}")

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def build(fed, scale):
        st.clear()
        torch.cuda.empty_cache()
        dim = FEDERATIONS[fed]["dim"]
        rows = [max(1, int(n * scale)) for n in FEDERATIONS[fed]["rows"]]
        begins, off = [], 0
        for n in rows:
            begins.append(off)
            off += -(-n // ALIGN) * ALIGN
        total = begins[-1] + rows[-1]
        g = torch.Generator(device=dev).manual_seed(7)
        xb = torch.zeros((total, dim), dtype=torch.float16, device=dev)
        hn = torch.zeros(total, dtype=torch.float32, device=dev)
        for b, n in zip(begins, rows):
            for s in range(0, n, 1 << 20):
                e = min(n, s + (1 << 20))
                xb[b + s: b + e] = (torch.randn((e - s, dim), generator=g, device=dev) / dim ** 0.5).half()
            ok(L.rr_half_sqnorms(xb[b: b + n].data_ptr(), 0, n, dim, hn[b: b + n].data_ptr(), stream()), "rr_half_sqnorms")
        xq = (torch.randn((NQ, dim), generator=g, device=dev) / dim ** 0.5).half()
        ws = torch.empty(L.rr_flat_search_workspace_bytes_for(K, dim), dtype=torch.uint8, device=dev)
        S = len(rows)
        nD = S * NQ * K * 4
        pad = (-nD) % 8
        packed = torch.empty(nD + pad + S * NQ * K * 8, dtype=torch.uint8, device=dev)      # [D f32 [S][nq][k] | pad | I i64 [S][nq][k]]
        segs = (Segment * S)(*[Segment(b, n, s << SHIFT, -1, 0) for s, (b, n) in enumerate(zip(begins, rows))])
        st.update(dim=dim, rows=rows, begins=begins, total=total, xb=xb, hn=hn, xq=xq, ws=ws, packed=packed, nD=nD, ioff=nD + pad, segs=segs,
                  D=torch.empty((NQ, K), dtype=torch.float32, device=dev), I=torch.empty((NQ, K), dtype=torch.int64, device=dev))
        torch.cuda.synchronize()
        return {"rows": rows, "dim": dim, "matrix_rows": total, "bytes": total * dim * 2}

    def search(mode):
        s, D, I = st, st["D"], st["I"]
        xb, hn, xq, ws, dim = s["xb"], s["hn"], s["xq"], s["ws"], s["dim"]
        if mode == "per_source_l2":
            S, pk = len(s["rows"]), s["packed"]
            for i, (b, n) in enumerate(zip(s["begins"], s["rows"])):
                ok(L.rr_flat_search_l2(xb[b: b + n].data_ptr(), hn[b: b + n].data_ptr(), 0, n, dim, xq.data_ptr(), NQ, K,
                                       pk.data_ptr() + i * NQ * K * 4, pk.data_ptr() + s["ioff"] + i * NQ * K * 8, i << SHIFT, ws.data_ptr(),
                                       ws.numel(), None, 0, stream()), "rr_flat_search_l2")
            ok(L.rr_merge_topk_gathered(pk.data_ptr(), 1, pk.numel(), s["ioff"], S, NQ, K, K, 0, D.data_ptr(), I.data_ptr(), stream()),
               "rr_merge_topk_gathered")
        elif mode == "seg_l2":
            ok(L.rr_flat_search_segments_l2(xb.data_ptr(), hn.data_ptr(), 0, s["total"], dim, s["segs"], len(s["rows"]), xq.data_ptr(), NQ, K,
                                            D.data_ptr(), I.data_ptr(), ws.data_ptr(), ws.numel(), None, 0, stream()), "rr_flat_search_segments_l2")
        elif mode == "seg_ip":
            ok(L.rr_flat_search_segments(xb.data_ptr(), 0, s["total"], dim, s["segs"], len(s["rows"]), xq.data_ptr(), NQ, K, D.data_ptr(),
                                         I.data_ptr(), ws.data_ptr(), ws.numel(), None, 0, stream()), "rr_flat_search_segments")
        elif mode == "plain_l2":      # the whole matrix as one corpus (gap rows are zero rows with zero norms)
            ok(L.rr_flat_search_l2(xb.data_ptr(), hn.data_ptr(), 0, s["total"], dim, xq.data_ptr(), NQ, K, D.data_ptr(), I.data_ptr(), 0,
                                   ws.data_ptr(), ws.numel(), None, 0, stream()), "rr_flat_search_l2")
        elif mode == "plain_ip":
            ok(L.rr_flat_search(xb.data_ptr(), 0, s["total"], dim, xq.data_ptr(), NQ, K, D.data_ptr(), I.data_ptr(), 0, ws.data_ptr(),
                                ws.numel(), None, 0, stream()), "rr_flat_search")
        else:
            raise ValueError(mode)

    for line in sys.stdin:
        c = json.loads(line)
        if c["cmd"] == "quit":
            break
        if c["cmd"] == "build":
            out = build(c["fed"], c["scale"])
        elif c["cmd"] == "ids":
            search(c["mode"])
            torch.cuda.synchronize()
            np.save(c["out"] + "_I.npy", st["I"].cpu().numpy())
            np.save(c["out"] + "_D.npy", st["D"].cpu().numpy())
            out = {"saved": c["out"]}
        elif c["cmd"] == "leg":
            for _ in range(3):
                search(c["mode"])
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(c["searches"]):
                search(c["mode"])
            b.record()
            torch.cuda.synchronize()
            out = {"mode": c["mode"], "searches": c["searches"], "ms_per_search": a.elapsed_time(b) / c["searches"]}
        else:
            raise ValueError(c["cmd"])
        print(json.dumps(out), flush=True)


# ---- parent ---------------------------------------------------------------------------------------------------------------------------
class Child:
    def __init__(self, lib):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", lib], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True, cwd=ROOT)

    def ask(self, **cmd):
        self.p.stdin.write(json.dumps(cmd) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"worker exited with status {self.p.wait()} on {cmd}")
        return json.loads(line)

    def close(self, kill=False):
        if self.p.poll() is None:
            if kill:
                self.p.kill()
            else:
                self.p.stdin.write('{"cmd": "quit"}\n')
                self.p.stdin.flush()
        self.p.wait()


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--baseline-lib", help="libragroute_hip.so built from the commit before rr_flat_search_segments_l2")
    ap.add_argument("--lib", default=os.path.join(ROOT, "ragroute_amd", "libragroute_hip.so"))
    ap.add_argument("--searches", type=int, default=50)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--feds", default="wikipedia,uae")
    ap.add_argument("--scale", type=float, default=1.0, help="row-count factor (rehearsals; 1.0 = the workloads as stated)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segments_l2"))
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    if not a.baseline_lib or not os.path.exists(a.baseline_lib) or not os.path.exists(a.lib):
        raise SystemExit("segments_l2_perf: --baseline-lib (the old library) and --lib must exist")
    import numpy as np
    os.makedirs(a.out, exist_ok=True)
    old, new = Child(os.path.abspath(a.baseline_lib)), Child(os.path.abspath(a.lib))
    results, failed = [], False
    try:
        for fed in a.feds.split(","):
            shape = old.ask(cmd="build", fed=fed, scale=a.scale)
            assert new.ask(cmd="build", fed=fed, scale=a.scale) == shape
            tmp = os.path.join(a.out, f"_{fed}")
            old.ask(cmd="ids", mode="per_source_l2", out=tmp + "_old")
            new.ask(cmd="ids", mode="seg_l2", out=tmp + "_new")
            I0, I1, D0, D1 = (np.load(tmp + s) for s in ("_old_I.npy", "_new_I.npy", "_old_D.npy", "_new_D.npy"))
            for s in ("_old_I.npy", "_new_I.npy", "_old_D.npy", "_new_D.npy"):
                os.remove(tmp + s)
            same = {"ids_identical": bool(np.array_equal(I0, I1)), "distances_identical": bool(np.array_equal(D0, D1)),
                    "ids_differing": int((I0 != I1).sum()), "max_abs_distance_diff": float(np.abs(D0 - D1).max())}
            legs = {m: [] for m in ("per_source_l2", "seg_l2", "seg_ip", "plain_l2", "plain_ip")}
            for _ in range(a.alternations):
                legs["per_source_l2"].append(old.ask(cmd="leg", mode="per_source_l2", searches=a.searches)["ms_per_search"])
                for m in ("seg_l2", "seg_ip", "plain_l2", "plain_ip"):
                    legs[m].append(new.ask(cmd="leg", mode=m, searches=a.searches)["ms_per_search"])
            base, seg = legs["per_source_l2"], legs["seg_l2"]
            spread = max(base) - min(base)
            r = {"federation": fed, "note": FEDERATIONS[fed]["note"], "scale": a.scale, **shape, "nq": NQ, "k": K, "searches_per_leg": a.searches,
                 "alternations": a.alternations, **same, "legs_ms_per_search": legs, "median_ms": {m: median(v) for m, v in legs.items()},
                 "baseline_spread_ms": spread, "segmented_minus_per_source_ms": median(seg) - median(base),
                 "not_slower_than_baseline_plus_spread": bool(median(seg) <= median(base) + spread),
                 "seg_l2_over_seg_ip": median(seg) / median(legs["seg_ip"]), "plain_l2_over_plain_ip": median(legs["plain_l2"]) / median(legs["plain_ip"])}
            failed |= not (same["ids_identical"] and r["not_slower_than_baseline_plus_spread"])
            results.append(r)
            print(json.dumps(r), flush=True)
        old.close()
        new.close()
    except BaseException:
        old.close(kill=True)
        new.close(kill=True)
        raise
    with open(os.path.join(a.out, "segments_l2_perf.json"), "w") as f:
        json.dump({"tool": "tools/segments_l2_perf.py", "time": time.strftime("%Y-%m-%d %H:%M:%S"), "results": results}, f, indent=1)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
