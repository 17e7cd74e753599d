"""The measurement panda_ntt_execute_batch stands on: `batch` forward transforms of 2^log_n points over one field with one root, as
  arm A: `batch` successive panda_ntt_execute_<field>_v1 calls (symbols every build exports: --lib PATH runs this arm against another build), and
  arm F: ONE panda_ntt_execute_batch call.
One process, data resident, the two arms' outputs compared byte for byte before anything is timed, every shape warmed up (tables cached),
wall clock around calls that end in the library's own synchronise, the arms alternated --alternations times, each arm timed over enough
calls to last --min-seconds.  One JSON line per configuration with the per-member milliseconds of every repetition.

usage: batch_ntt_bench.py [--lib PATH] [--arms AF|A] [--configs field:log_n:batch,...] [--alternations N] [--min-seconds S] [--out FILE]
                          [--baseline FILE]   (JSON lines of an arm-A run of another build: prints the verdicts of DESIGN.md "Batched NTT")"""
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

DEFAULT_CONFIGS = "0:8:4096,0:12:256,0:16:64,0:16:13,0:18:16,0:20:16,0:24:2,2:16:64"
ENTRY = ("panda_ntt_execute_bn254_v1", "panda_ntt_execute_bls12_377_v1", "panda_ntt_execute_bls12_381_v1")


def device_line(lib, single, cfg):
    """device name and the shader clock one call ran at (panda_set_clock_stamps, as bench.py records it)"""
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        name = f"{p.name} ({getattr(p, 'gcnArchName', '?').split(':')[0]}, {p.multi_processor_count} CUs)"
    except Exception as e:  # noqa: BLE001
        name = f"unknown ({type(e).__name__})"
    mhz = None
    if hasattr(lib, "panda_set_clock_stamps"):
        lib.panda_set_clock_stamps(1)
        clk = (C.c_uint64 * ffi.CLOCK_WORDS)()
        ffi.check(single(cfg), "ntt")
        lib.panda_ntt_last_clock(clk)
        lib.panda_set_clock_stamps(0)
        if clk[1]:
            mhz = round(int(clk[3]) / int(clk[1]) * 100.0)
    return name, mhz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--arms", default="AF")
    ap.add_argument("--configs", default=DEFAULT_CONFIGS)
    ap.add_argument("--alternations", type=int, default=10)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--out")
    ap.add_argument("--baseline")
    a = ap.parse_args()
    if a.lib:
        ffi.LIB_PATH = os.path.abspath(a.lib)
    import numpy as np
    import oracle as po
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    arms = [x for x in a.arms if x in "AF"]
    if "F" in arms and not hasattr(lib, "panda_ntt_execute_batch"):
        raise SystemExit("this build has no panda_ntt_execute_batch: run it with --arms A")
    baseline = {}
    if a.baseline:
        for line in open(a.baseline):
            if line.startswith("{"):
                r = json.loads(line)
                baseline[(r["field"], r["log_n"], r["batch"])] = r
    gm = pgm.PandaGpuManager(0)
    out = open(a.out, "a") if a.out else None
    try:
        for spec in a.configs.split(","):
            field, k, batch = (int(x) for x in spec.split(":"))
            n = 1 << k
            single = getattr(lib, ENTRY[field])
            omega = po.root_of_unity(po.FR_OF[field], k)
            om = C.c_void_p(omega.ctypes.data)
            src = {arm: DeviceBuffer(batch * n * 32) for arm in arms}
            dst = {arm: DeviceBuffer(batch * n * 32) for arm in arms}
            flags = {arm: C.c_uint(9) for arm in "AF"}
            try:
                def fill():
                    for arm in arms:
                        ffi.check(lib.panda_gen_scalars(field, 0x5EED + k, 0, batch * n, src[arm].ptr, NULL_STREAM), "gen")
                    ffi.check(lib.panda_stream_sync(NULL_STREAM), "sync")

                mk = lambda s, d, f: ffi.NttconfigurationV1(gm.mem_pool, gm.exec_stream.raw, s, d, om, k, C.pointer(f))
                cfg_members = [mk(C.c_void_p(src["A"].ptr.value + j * n * 32), C.c_void_p(dst["A"].ptr.value + j * n * 32), flags["A"]) for j in range(batch)] if "A" in arms else []
                cfg_batch = mk(src["F"].ptr, dst["F"].ptr, flags["F"]) if "F" in arms else None

                def run_a():
                    for c in cfg_members:
                        ffi.check(single(c), "ntt")

                def run_f():
                    ffi.check(lib.panda_ntt_execute_batch(field, 0, cfg_batch, batch, None), "batch")

                run = {"A": run_a, "F": run_f}
                launches = members_per_workgroup = None
                if "F" in arms:
                    ln, mp = C.c_uint(0), C.c_uint(0)
                    ffi.check(lib.panda_ntt_batch_plan(k, 0, batch, C.byref(ln), C.byref(mp)), "plan")
                    launches, members_per_workgroup = ln.value, mp.value
                # the outputs of the two arms on the same input, byte for byte, before anything is timed
                fill()
                for arm in arms:
                    run[arm]()
                if len(arms) == 2:
                    if flags["A"].value != flags["F"].value:
                        raise SystemExit(f"field {field} 2^{k} x {batch}: the arms' flags differ")
                    ra = (dst if flags["A"].value else src)["A"].to_host(np.uint8)
                    rf = (dst if flags["F"].value else src)["F"].to_host(np.uint8)
                    if not np.array_equal(ra, rf):
                        raise SystemExit(f"field {field} 2^{k} x {batch}: the arms' outputs differ")
                    del ra, rf
                # warm-up of every shape (tables are cached from here on); a transform's input may be any canonical data, so the
                # timed calls keep transforming what the calls before them left in src
                reps = {}
                for arm in arms:
                    run[arm]()
                    t0 = time.perf_counter()
                    run[arm]()
                    reps[arm] = max(1, int(a.min_seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
                name, mhz = device_line(lib, single, mk(src[arms[0]].ptr, dst[arms[0]].ptr, flags[arms[0]]))
                ms = {arm: [] for arm in arms}
                for _ in range(a.alternations):
                    for arm in arms:
                        t0 = time.perf_counter()
                        for _ in range(reps[arm]):
                            run[arm]()
                        ms[arm].append((time.perf_counter() - t0) / (reps[arm] * batch) * 1e3)
                rec = {"field": field, "log_n": k, "batch": batch, "launches": launches, "members_per_workgroup": members_per_workgroup,
                       "device": name, "sclk_mhz": mhz, "lib": "in-tree" if not a.lib else os.path.basename(os.path.dirname(ffi.LIB_PATH)) + "/" + os.path.basename(ffi.LIB_PATH),
                       "calls_per_repetition": reps, "per_member_ms": {arm: [round(v, 6) for v in ms[arm]] for arm in arms}}
                for arm in arms:
                    v = ms[arm]
                    rec[f"{arm}_min_med_max"] = [round(min(v), 6), round(statistics.median(v), 6), round(max(v), 6)]
                if "A" in arms and "F" in arms:
                    rec["F_over_A_median"] = round(statistics.median(ms["F"]) / statistics.median(ms["A"]), 4)
                base = baseline.get((field, k, batch))
                if base:
                    bmin, bmed, bmax = base["A_min_med_max"]
                    rec["baseline_A_min_med_max"] = base["A_min_med_max"]
                    if "F" in arms:
                        rec["F_median_over_baseline_median"] = round(statistics.median(ms["F"]) / bmed, 4)
                        rec["F_slowest_beats_baseline_fastest"] = max(ms["F"]) < bmin
                        rec["F_median_within_baseline_spread"] = statistics.median(ms["F"]) <= bmed + (bmax - bmin)
                    if "A" in arms:
                        rec["A_median_within_baseline_spread"] = abs(statistics.median(ms["A"]) - bmed) <= bmax - bmin
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            finally:
                for d in list(src.values()) + list(dst.values()):
                    d.free()
    finally:
        if out:
            out.close()
        gm.deinit()


if __name__ == "__main__":
    main()
