"""Cases and runners of the wide-value parity tests (tests/test_wide_values_gpu.py) and the table of (d, family, dtype) cells
that tests/test_wide_values_data.py proves exact, order independent and sensitive on the CPU.

The data are tests/util.py's exact families: integer valued, every significant bit of fp16 / bf16 in use, power-of-two row scales
in the scaled family - ids and scores must equal the f64 oracle bit for bit, and would not if a kernel dropped a mantissa bit.

Cost: the oracle's work n * d * nq per search stays under fuzz_cases.cases' bounds (6e9; 3e10 for the chunked corpora, as its
`big` sample).  Row counts are what was cut to fit the suite's time, never the kernel x mode x family x dtype coverage."""
import math

import numpy as np

KERNELS = {"flat_scan16_kernel", "flat_scan16h_kernel", "flat_scan_wide_pd_kernel", "flat_scan_wide8_kernel", "flat_scan_wide_rs_kernel"}
DTYPES = ("fp16", "bf16")
IP_FAMILIES = ("rows", "queries", "balanced", "scaled")
FAMILIES = IP_FAMILIES + ("l2",)
MAX_WORK, MAX_WORK_CHUNKED = 6e9, 3e10

# (d, query counts): padded widths (8, 100 -> 128; 769 -> 896), every width class up to 8192, query counts on both sides of the
# 64 / 128 / 192 / 208-209 / 256 boundaries and beyond one 256-query block
GRID = [(8, (1,)), (100, (63, 64)), (384, (257,)), (768, (65, 256)),                       # query-resident rows
        (769, (17, 128)), (1024, (127, 129, 192, 193, 208, 209, 256)), (1536, (64,)),              # half-resident below 129 queries
        (1664, (64,)), (2048, (128, 191, 300)), (4096, (192, 193)), (8192, (3, 256))]              # wide rows only
# one (d, query counts) per kernel for the chunk schedule, chosen for the cheapest oracle: (rows, k) give bootstrap + two chunk
# launches (capi.hip chunk_schedule: few rows need a large k for a second chunk), which run_flat_case asserts
CHUNKED = [(384, (65,), 35_000, 300),            # flat_scan16_kernel
           (769, (17, 209), 24_000, 600),         # flat_scan16h_kernel; flat_scan_wide_rs_kernel (L2: its L2 form at 209 queries)
           (1664, (5, 130), 24_000, 600),         # flat_scan_wide8_kernel (one 16-query block); flat_scan_wide_pd_kernel (nine blocks)
           (2176, (3,), 24_000, 600)]             # flat_scan_wide_pd_kernel above 2048
CHUNKED_8192 = (8192, (3,), 24_001, 1024)        # rows family only, both dtypes: the widest row through chunk launches
# more chunk-launch shapes of the two kernels that only run there, on two (family, dtype) pairs each: the 8-wave kernel with two
# 16-query blocks per wave (100 queries), the row-split kernel at 2048 and above it (256 / 193 queries)
CHUNKED_EXTRA = [(2048, (100, 256), 24_000, 600), (4096, (193,), 24_000, 600)]
CHUNKED_EXTRA_DATA = (("rows", "fp16"), ("l2", "bf16"))
FUZZ_WIDE_FLAT, FUZZ_WIDE_SEGMENTED = 60, 30     # cases of the fuzz samples that tests/test_fuzz_gpu.py also runs on wide values


def dense_rows(d, nqs):
    """Rows of a dense-path corpus (<= 8192): ragged (not a multiple of 32) and small enough for the oracle."""
    if d == 8:
        return 301
    if d == 768:
        return 8192                                   # the dense path's last size
    return min(3001, int(6e8 // (d * max(nqs))) | 1)


def flat_cases():
    """Every flat case: dict(d, n, k, nqs, family, dtype, metric, mode, seed)."""
    out = []
    for d, nqs in GRID:
        for fam in FAMILIES:
            for dt in DTYPES:
                out.append({"d": d, "n": dense_rows(d, nqs), "k": 10, "nqs": nqs, "family": fam, "dtype": dt, "mode": "dense"})
    for d, nqs, n, k in CHUNKED:
        for fam in FAMILIES:
            for dt in DTYPES:
                out.append({"d": d, "n": n, "k": k, "nqs": nqs, "family": fam, "dtype": dt, "mode": "chunked"})
    d, nqs, n, k = CHUNKED_8192
    for dt in DTYPES:
        out.append({"d": d, "n": n, "k": k, "nqs": nqs, "family": "rows", "dtype": dt, "mode": "chunked"})
    for d, nqs, n, k in CHUNKED_EXTRA:
        for fam, dt in CHUNKED_EXTRA_DATA:
            out.append({"d": d, "n": n, "k": k, "nqs": nqs, "family": fam, "dtype": dt, "mode": "chunked"})
    for i, c in enumerate(out):
        c["metric"] = "l2" if c["family"] == "l2" else "ip"
        c["seed"] = 20261017 + i
        for nq in c["nqs"]:
            assert c["n"] * c["d"] * nq <= (MAX_WORK if c["mode"] == "dense" else MAX_WORK_CHUNKED), c
    return out


# segmented searches: (d, rows per source, query counts, k); 768 is query-resident, 2048 wide (200 / 209 queries: 8-wave / row-split)
SEGMENT_CASES = [(768, [9_000, 31, 0, 257, 12_000], (16, 256), 32),
                 (2048, [3_000, 31, 257, 9_000], (200, 209), 10),
                 (768, [300, 5, 4_100], (40,), 10)]                       # under 8192 rows in total: the dense path
SEGMENT_DATA = {"ip": (("rows", "fp16"), ("scaled", "bf16"), ("balanced", "bf16"), ("queries", "fp16")),
                "l2": (("l2", "fp16"), ("l2", "bf16"))}
SCREEN_CASES = [(768, 20_000, 40, 10), (1024, 9_001, 130, 32), (100, 3_000, 7, 10)]     # (d, n, nq, k): d <= 1536
SUBNORMAL_CASES = [(768, (5, 256)), (2048, (5, 256))]                                   # fp16; a small and a full query block


def cells():
    """Every (d, family, dtype) whose data a GPU test uses: what the CPU tests of the data cover."""
    out = {(c["d"], c["family"], c["dtype"]) for c in flat_cases()}
    for d, _, _, _ in SEGMENT_CASES:
        out |= {(d, fam, dt) for pairs in SEGMENT_DATA.values() for fam, dt in pairs}
    for d, _, _, _ in SCREEN_CASES:
        out |= {(d, fam, dt) for fam in IP_FAMILIES for dt in DTYPES}
    return sorted(out | fuzz_cells())


def fuzz_cells():
    """The (d, family, dtype) of the wide-value fuzz runs of tests/test_fuzz_gpu.py (the family comes from each case's seed)."""
    from tests import fuzz_cases as F
    out = {(c["d"], F.wide_family(c, c["metric"]), c["dtype"]) for c in F.cases(20261004, FUZZ_WIDE_FLAT)}
    for c in F.segment_cases(20261006, FUZZ_WIDE_SEGMENTED):
        out |= {(c["d"], F.wide_family(c, m), c["dtype"]) for m in ("ip", "l2")}
    return out


HALF_RESIDENT_DIMS = (896, 1024, 1280, 1536)


DENSE_FORMS = {"flat_scan16_kernel", "flat_scan16h_kernel", "flat_scan_wide_pd_kernel"}


def kernel_coverage(lib):
    """{kernel name: {(mode, dtype, family)}} of the flat cases.  rr_flat_scan_kernel_name(dim, queries of the block) reports the plan
    of the FILTER (chunk) launches of an inner-product search.  A dense launch (a corpus of <= 8192 rows, and every bootstrap) of a
    wide row always runs the 4-wave kernel, whatever the report says: the 8-wave and row-split kernels have no dense form, so a dense
    case that the report assigns to them is counted for flat_scan_wide_pd_kernel.  An L2 search differs from the report only at the
    half-resident widths below 129 queries (it goes to a wide-row kernel there), so those L2 runs are left out of the table."""
    reached = {}
    for c in flat_cases():
        dim = lib.rr_padded_dim(c["d"])
        for nq in c["nqs"]:
            for block in {min(nq, 256), nq % 256 or 256}:                     # a 300-query call: blocks of 256 and 44
                if c["metric"] == "l2" and dim in HALF_RESIDENT_DIMS and block < 129:
                    continue
                name = lib.rr_flat_scan_kernel_name(dim, block).decode()
                if c["mode"] == "dense" and name not in DENSE_FORMS and name in KERNELS:
                    name = "flat_scan_wide_pd_kernel"
                reached.setdefault(name, set()).add((c["mode"], c["dtype"], c["family"]))
    return reached


def assert_kernel_coverage(lib):
    """All five names and no sixth; each kernel in both storage types with every family it serves, in chunk launches and - the
    three kernels that have one - in its dense form."""
    reached = kernel_coverage(lib)
    assert set(reached) == KERNELS, sorted(reached)
    for name, combos in sorted(reached.items()):
        fams = IP_FAMILIES if name == "flat_scan16h_kernel" else FAMILIES      # (the half-resident kernel has no L2 form)
        modes = ("dense", "chunked") if name in DENSE_FORMS else ("chunked",)
        missing = {(m, t, f) for m in modes for t in DTYPES for f in fams} - combos
        assert not missing, (name, sorted(missing))
        assert name in DENSE_FORMS or not any(m == "dense" for m, _, _ in combos)
    return reached


def _scan_launches(fn):
    """fn() under the library's launch profile: (result, scan launches made)."""
    import ctypes
    from ragroute_amd import _lib
    L = _lib.lib()
    _lib.check(L.rr_profile_begin(4096), "rr_profile_begin")
    try:
        res = fn()
    finally:
        ms, n, rows = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        _lib.check(L.rr_profile_end(ctypes.byref(ms), ctypes.byref(n), ctypes.byref(rows)), "rr_profile_end")
    return res, n.value


def run_flat_case(c, dev):
    """One flat case -> list of the query counts that failed.  dense: the public f32 surface (FlatIndex.add / search); chunked:
    search_prepared on the guard-page layout (corpus and queries end on the last mapped byte: an over-read faults).  The scan
    launches are counted: one per query block on the dense path, bootstrap + at least two chunk launches on the other."""
    import torch
    from oracle import oracle as O
    from ragroute_amd.flat_index import FlatIndex
    from tests.test_guard_pages_gpu import _flush_to_end
    from tests.util import exact_case
    rng = np.random.default_rng(c["seed"])
    d, n, k = c["d"], c["n"], c["k"]
    xb, xq_all = exact_case(rng, n, max(c["nqs"]), d, c["family"], c["dtype"])
    idx = FlatIndex(d, metric=c["metric"], dtype=c["dtype"], device=dev)
    tdt = torch.float16 if c["dtype"] == "fp16" else torch.bfloat16
    search = O.flat_search_l2 if c["metric"] == "l2" else O.flat_search_ip
    keep_b = None
    if c["mode"] == "dense":
        idx.add(xb)
    else:
        xb_h = torch.zeros((n, idx.dim), dtype=tdt)
        xb_h[:, :d] = torch.from_numpy(xb).to(tdt)
        keep_b, xb_dev = _flush_to_end(xb_h, dev)
        del xb_h
        idx.adopt(xb_dev)
    bad = []
    for nq in c["nqs"]:
        xq = xq_all[:nq]
        blocks = math.ceil(nq / 256)
        if c["mode"] == "dense":
            (D, I), launches = _scan_launches(lambda: idx.search(xq, k))
            ok_launches = launches == blocks
        else:
            xq_h = torch.zeros((nq, idx.dim), dtype=tdt)
            xq_h[:, :d] = torch.from_numpy(xq).to(tdt)
            keep_q, xq_dev = _flush_to_end(xq_h, dev)
            (D, I), launches = _scan_launches(lambda: idx.search_prepared(xq_dev, k))
            torch.cuda.synchronize()
            D, I = D.cpu().numpy(), I.cpu().numpy()
            del keep_q
            ok_launches = launches >= 3 * blocks
        Dr, Ir = search(xb, xq, k)
        ok = np.array_equal(I, Ir) and np.array_equal(D, Dr)
        if not (ok and ok_launches):
            print("MISMATCH" if not ok else "SCHEDULE", c, "nq", nq, "launches", launches,
                  "queries with wrong ids", int((I != Ir).any(1).sum()), "with wrong scores", int((D != Dr).any(1).sum()), flush=True)
            bad.append(nq)
    del keep_b
    return bad


def run_subnormal_case(d, nqs, dev, n=9_001, k=10):
    """fp16 rows that are mostly SUBNORMAL (tests/util.py subnormal_case) through add / search (the library's own f32 -> fp16
    conversion) on the dense path and through adopt / search_prepared (host conversion) on a chunked corpus -> list of failures."""
    import torch
    from oracle import oracle as O
    from ragroute_amd.flat_index import FlatIndex
    from tests.util import half_round, subnormal_case
    rng = np.random.default_rng(d)
    xb, xq_all, pure = subnormal_case(rng, n, max(nqs), d)
    assert np.array_equal(half_round(xb), xb) and np.array_equal(half_round(xq_all), xq_all)
    bad = []
    for rows, surface in ((3_001, "add"), (n, "adopt")):
        idx = FlatIndex(d, dtype="fp16", device=dev)
        if surface == "add":
            idx.add(xb[:rows])
            assert np.array_equal(idx.xb[:, :d].float().cpu().numpy(), xb[:rows]), "rr_rows_to_half changed a subnormal value"
        else:
            idx.adopt(torch.from_numpy(xb[:rows]).to(torch.float16).to(dev))
        for nq in nqs:
            Dr, Ir = O.flat_search_ip(xb[:rows], xq_all[:nq], k)
            if surface == "add":
                D, I = idx.search(xq_all[:nq], k)
            else:
                D, I = (t.cpu().numpy() for t in idx.search_prepared(torch.from_numpy(xq_all[:nq]).to(torch.float16).to(dev), k))
            assert pure[Ir].any() and not pure[Ir].all(), "the ranking should cross the subnormal boundary"
            if not (np.array_equal(I, Ir) and np.array_equal(D, Dr)):
                print("MISMATCH subnormal", d, rows, surface, nq, "wrong ids", int((I != Ir).any(1).sum()), "wrong scores",
                      int((D != Dr).any(1).sum()), "max |D - Dref| / |Dref|", float(np.abs((D - Dr) / Dr).max()), flush=True)
                bad.append((rows, surface, nq))
    return bad
