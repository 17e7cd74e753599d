"""The measurement panda_sparse_matvec stands on.  BN254 Fr; the CSR structure is generated with numpy from a seed, the values and the
vector with panda_gen_scalars.  n_cols = n_rows everywhere.
  uniform    2^20, 2^22, 2^24 rows of 4 nonzeros, columns uniform at random
  skewed, each at 2^24 nonzeros and compared with the uniform matrix of 2^24 nonzeros:
    heavy1pct   1 % of 2^22 rows hold half the nonzeros
    onerow      one of 2^22 rows holds a quarter of all nonzeros
    halfempty   2^23 rows, every other one empty
    constwire   2^22 rows of 4 whose first nonzero names column 0 (the constant wire)
  rows3 (not run by default): 2^24 nonzeros in rows of 3, which do not line up with the four nonzeros of a thread
Arms, alternated --alternations times, each timed over enough runs to last --min-seconds (milliseconds per run):
  M  one device-to-device panda_memcpy that moves the product's own traffic, 36 nnz + 4 (n_rows + 1) + 32 n_cols + 32 n_rows bytes (half of
     them copied: a copy reads and writes every byte), followed by a synchronise as every library call ends in one
  P  panda_sparse_matvec, batch 1          C  panda_sparse_check alone
  B  panda_sparse_matvec, batch 4          S  four calls of batch 1 on the same four vectors
  m  arm M again (the A/A of the baseline: its run-to-run spread in the same alternation)
Before anything is timed the structure must pass panda_sparse_check, and a sample of rows of at most 4096 nonzeros is compared with
Python integers; arm B's output is compared byte for byte with arm S's.  One JSON line per configuration, then a table.

usage: sparse_bench.py [--cases uniform20,uniform22,uniform24,heavy1pct,onerow,halfempty,constwire] [--alternations N] [--min-seconds S] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from panda_amd import gpu_ffi as ffi  # noqa: E402

FIELD = 0
W = 1 << 256
R_BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SKEW_NNZ = 1 << 24
ALL_CASES = "uniform20,uniform22,uniform24,heavy1pct,onerow,halfempty,constwire"


def device_name():
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        return f"unknown ({type(e).__name__})"


def structure(case, seed=0x5BA25E):
    """-> (row lengths, columns) as numpy arrays; n_cols = n_rows"""
    import numpy as np
    rng = np.random.default_rng(seed)

    def spread(total, rows):  # `total` nonzeros over `rows` rows, as evenly as integers allow
        lengths = np.full(rows, total // rows, np.int64)
        lengths[:total % rows] += 1
        return lengths

    if case.startswith("uniform"):
        n_rows = 1 << int(case[len("uniform"):])
        lengths = np.full(n_rows, 4, np.int64)
    elif case == "heavy1pct":
        n_rows = 1 << 22
        heavy = n_rows // 100
        lengths = np.empty(n_rows, np.int64)
        mask = np.zeros(n_rows, bool)
        mask[rng.choice(n_rows, heavy, replace=False)] = True
        lengths[mask] = spread(SKEW_NNZ // 2, heavy)
        lengths[~mask] = spread(SKEW_NNZ // 2, n_rows - heavy)
    elif case == "onerow":
        n_rows = 1 << 22
        lengths = np.empty(n_rows, np.int64)
        mask = np.zeros(n_rows, bool)
        mask[12345] = True
        lengths[mask] = SKEW_NNZ // 4
        lengths[~mask] = spread(SKEW_NNZ - SKEW_NNZ // 4, n_rows - 1)
    elif case == "halfempty":
        n_rows = 1 << 23
        lengths = np.zeros(n_rows, np.int64)
        lengths[0::2] = 4
    elif case == "constwire":
        n_rows = 1 << 22
        lengths = np.full(n_rows, 4, np.int64)
    elif case == "rows3":  # not a default case: uniform rows that do not line up with a thread's four nonzeros
        n_rows = -(-SKEW_NNZ // 3)
        lengths = np.full(n_rows, 3, np.int64)
        lengths[-1] = SKEW_NNZ - 3 * (n_rows - 1)
    else:
        raise SystemExit(f"unknown case {case}")
    nnz = int(lengths.sum())
    col = rng.integers(0, n_rows, nnz, dtype=np.uint32)
    if case == "constwire":
        col[0::4] = 0
    return lengths, col


def measure(run, arms, alternations, min_seconds):
    """run: {arm: callable} -> per-arm lists of ms per run, alternated"""
    reps = {}
    for arm in arms:
        run[arm]()
        t0 = time.perf_counter()
        run[arm]()
        reps[arm] = max(1, int(min_seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
    ms = {arm: [] for arm in arms}
    for _ in range(alternations):
        for arm in arms:
            t0 = time.perf_counter()
            for _ in range(reps[arm]):
                run[arm]()
            ms[arm].append((time.perf_counter() - t0) / reps[arm] * 1e3)
    return ms


def table(recs):
    uniform = {r["nnz"]: r["median_ms"]["P"] for r in recs if r["case"].startswith("uniform")}
    lines = ["case        rows      nnz       traffic MiB | copy M ms   m ms     spread | product ms  x copy  x uniform | check ms  x copy | batch 4 ms  4 singles ms"]
    for r in recs:
        med = r["median_ms"]
        base = uniform.get(r["nnz"])
        lines.append("%-11s %-9d %-9d %11.1f | %9.4f %9.4f %7.4f | %10.4f %7.2f %10s | %8.4f %7.2f | %10s  %12s" % (
            r["case"], r["n_rows"], r["nnz"], r["traffic_bytes"] / 2**20, med["M"], med["m"], r["copy_spread_ms"], med["P"], r["product_to_copy"],
            "%.3f" % (med["P"] / base) if base else "-", med["C"], r["check_to_copy"], "%.4f" % med["B"] if "B" in med else "-",
            "%.4f" % med["S"] if "S" in med else "-"))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=ALL_CASES)
    ap.add_argument("--batch-case", default="uniform22", help="the case that also times batch 4 against four single calls")
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    gm = pgm.PandaGpuManager(0)
    stream = gm.exec_stream.raw
    out_file = open(a.out, "a") if a.out else None
    recs = []
    name = device_name()
    tile, chunk = C.c_uint(0), C.c_uint(0)
    ffi.check(lib.panda_sparse_plan(8, 8, 8, 1, C.byref(tile), C.byref(chunk), None, None), "plan")

    def emit(rec):
        recs.append(rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if out_file:
            out_file.write(line + "\n")
            out_file.flush()

    def fetch(buf, index, count=1):
        words = np.empty((count, 8), np.uint32)
        ffi.check(lib.panda_memcpy(C.c_void_p(words.ctypes.data), C.c_void_p(buf.ptr.value + 32 * index), 32 * count), "memcpy")
        raw = words.tobytes()
        winv = pow(W, -1, R_BN254)
        return [int.from_bytes(raw[32 * j:32 * j + 32], "little") * winv % R_BN254 for j in range(count)]

    try:
        for case in a.cases.split(","):
            lengths, col = structure(case)
            n_rows = n_cols = len(lengths)
            nnz = len(col)
            row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
            batch = 4 if case == a.batch_case else 1
            traffic = 36 * nnz + 4 * (n_rows + 1) + 32 * n_cols + 32 * n_rows
            bufs = {"rp": DeviceBuffer.from_host(row_ptr), "cl": DeviceBuffer.from_host(col), "vl": DeviceBuffer(32 * nnz), "z": DeviceBuffer(32 * n_cols * batch),
                    "out": DeviceBuffer(32 * n_rows * batch), "out2": DeviceBuffer(32 * n_rows * batch), "src": DeviceBuffer(traffic // 2 + 32),
                    "dst": DeviceBuffer(traffic // 2 + 32)}
            try:
                ffi.check(lib.panda_gen_scalars(FIELD, 0x7A, 0, nnz, bufs["vl"].ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_gen_scalars(FIELD, 0x7B, 0, n_cols * batch, bufs["z"].ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_gen_scalars(FIELD, 0x7C, 0, traffic // 64 + 1, bufs["src"].ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")
                m = ffi.CsrMatrix(bufs["rp"].ptr.value, bufs["cl"].ptr.value, bufs["vl"].ptr.value, n_rows, n_cols, nnz)

                def product(out=bufs["out"], z_offset=0, out_offset=0, members=1):
                    ffi.check(lib.panda_sparse_matvec(FIELD, C.byref(m), C.c_void_p(bufs["z"].ptr.value + z_offset), C.c_void_p(out.ptr.value + out_offset), members,
                                                      stream), "matvec")

                def check():
                    d, w = C.c_uint(9), C.c_uint64(0)
                    ffi.check(lib.panda_sparse_check(FIELD, C.byref(m), C.byref(d), C.byref(w), stream), "check")
                    return d.value, w.value

                def copy():
                    ffi.check(lib.panda_memcpy(bufs["dst"].ptr, bufs["src"].ptr, traffic // 2), "copy")
                    ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")

                if check()[0] != 0:
                    raise SystemExit(f"{case}: the generated structure does not pass the check: {check()}")
                product()
                rng = np.random.default_rng(7)
                sample = [int(r) for r in rng.integers(0, n_rows, 400) if lengths[r] <= 4096][:48] + [0, n_rows - 1]
                for r in sample:
                    k0, k1 = int(row_ptr[r]), int(row_ptr[r + 1])
                    vals = fetch(bufs["vl"], k0, k1 - k0) if k1 > k0 else []
                    want = sum(v * fetch(bufs["z"], int(col[k0 + j]))[0] for j, v in enumerate(vals)) % R_BN254
                    if fetch(bufs["out"], r)[0] != want:
                        raise SystemExit(f"{case}: row {r} differs from the definition")
                run = {"M": copy, "P": product, "C": check, "m": copy}
                arms = "MPCm"
                if batch > 1:
                    def together():
                        product(members=batch)

                    def singles():
                        for p in range(batch):
                            product(bufs["out2"], 32 * n_cols * p, 32 * n_rows * p)

                    together()
                    singles()
                    if not np.array_equal(bufs["out"].to_host(), bufs["out2"].to_host()):
                        raise SystemExit(f"{case}: the batched product differs from the single calls")
                    run.update({"B": together, "S": singles})
                    arms = "MPCBSm"
                ms = measure(run, arms, a.alternations, a.min_seconds)
                med = {arm: statistics.median(ms[arm]) for arm in arms}
                spread = max(max(ms["M"]) - min(ms["M"]), max(ms["m"]) - min(ms["m"]), abs(med["M"] - med["m"]))
                emit({"case": case, "field": FIELD, "n_rows": n_rows, "n_cols": n_cols, "nnz": nnz, "longest_row": int(lengths.max()),
                      "empty_rows": int((lengths == 0).sum()), "tile": tile.value, "carry_chunk": chunk.value, "traffic_bytes": traffic, "device": name,
                      "verified_rows": len(sample), "per_run_ms": {arm: [round(v, 5) for v in ms[arm]] for arm in arms},
                      "median_ms": {arm: round(med[arm], 5) for arm in arms}, "copy_spread_ms": round(spread, 5),
                      "product_to_copy": round(med["P"] / med["M"], 4), "check_to_copy": round(med["C"] / med["M"], 4),
                      "gb_per_s": round(traffic / med["P"] / 1e6, 1)})
            finally:
                for b in bufs.values():
                    b.free()
        text = table(recs)
        print(text, flush=True)
        if out_file:
            out_file.write(text + "\n")
    finally:
        if out_file:
            out_file.close()
        gm.deinit()


if __name__ == "__main__":
    main()
