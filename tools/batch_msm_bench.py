"""The measurement panda_msm_execute_batch stands on: `batch` scalar vectors over one tabled base set, as
  arm A: `batch` successive panda_msm_execute_<curve> calls (symbols every build exports: --lib PATH runs this arm against another build), and
  arm F: ONE panda_msm_execute_batch call.
One process, tables precomputed, scalars resident, the two arms' outputs compared as affine points before anything is timed, every shape
warmed up, wall clock around calls that end in the library's own synchronise, the arms alternated --alternations times, each arm timed over
enough calls to last --min-seconds.  One JSON line per configuration with the per-member milliseconds of every repetition.

usage: batch_msm_bench.py [--lib PATH] [--arms AF|A] [--configs curve:log_n:batch,...] [--alternations N] [--min-seconds S] [--out FILE]
                          [--baseline FILE]   (JSON lines of an arm-A run of another build: prints the verdicts of DESIGN.md "Batched MSM")"""
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

DEFAULT_CONFIGS = "0:16:64,0:18:16,0:20:16,0:16:13,4:16:64,4:18:16,4:20:16,4:16:13"
ENTRY = {0: "panda_msm_execute_bn254", 4: "panda_msm_execute_bls12_381_g2"}
POINT_BYTES = {0: 64, 4: 192}
RESULT_BYTES = {0: 96, 4: 288}


def affine(curve, raw):
    import numpy as np
    if curve == 0:
        import oracle as po
        return po.to_affine(po.BN254, np.ascontiguousarray(raw).view(np.uint32)).tobytes()
    import pyref_bls381_g2 as g2
    return g2.decode(raw)


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
        ffi.check(single(cfg), "msm")
        lib.panda_msm_last_clock(clk)
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
    from gpu_util import NULL_STREAM, DeviceBuffer
    from panda_amd import gpu_manager as pgm
    lib = ffi.load()
    arms = [x for x in a.arms if x in "AF"]
    if "F" in arms and not hasattr(lib, "panda_msm_execute_batch"):
        raise SystemExit("this build has no panda_msm_execute_batch: run it with --arms A")
    baseline = {}
    if a.baseline:
        for line in open(a.baseline):
            if line.startswith("{"):
                r = json.loads(line)
                baseline[(r["curve"], r["log_n"], r["batch"])] = r
    gm = pgm.PandaGpuManager(0)
    out = open(a.out, "a") if a.out else None
    try:
        for spec in a.configs.split(","):
            curve, k, batch = (int(x) for x in spec.split(":"))
            n, res = 1 << k, RESULT_BYTES[curve]
            single = getattr(lib, ENTRY[curve])
            db, ds = DeviceBuffer(n * POINT_BYTES[curve]), DeviceBuffer(batch * n * 32)
            dr = {arm: DeviceBuffer(batch * res) for arm in "AF"}
            try:
                ffi.check(lib.panda_gen_bases(curve, 0x5EED + k, 0, n, db.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_gen_scalars(curve, 0x5EED + k + 1, 0, batch * n, ds.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_msm_precompute_bases(curve, db.ptr, k, 0, gm.exec_stream.raw), "precompute")
                tables, bits = C.c_uint(0), C.c_uint(0)
                ffi.check(lib.panda_msm_registered_info(db.ptr, C.byref(tables), C.byref(bits), None), "info")
                mk = lambda s, r: ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, db.ptr, s, r, k, pgm.JACOBIAN)
                cfg_members = [mk(C.c_void_p(ds.ptr.value + j * n * 32), C.c_void_p(dr["A"].ptr.value + j * res)) for j in range(batch)]
                cfg_batch = mk(ds.ptr, dr["F"].ptr)

                def run_a():
                    for c in cfg_members:
                        ffi.check(single(c), "msm")

                def run_f():
                    ffi.check(lib.panda_msm_execute_batch(curve, cfg_batch, batch), "batch")

                run = {"A": run_a, "F": run_f}
                group_log = sequences = None
                if "F" in arms:
                    gl, sq = C.c_uint(0), C.c_uint(0)
                    ffi.check(lib.panda_msm_batch_plan(curve, k, bits.value, batch, C.byref(gl), C.byref(sq)), "plan")
                    group_log, sequences = gl.value, sq.value
                # warm-up of every shape (the arena grows to its size here), then the outputs of the two arms as affine points
                reps = {}
                for arm in arms:
                    run[arm]()
                    t0 = time.perf_counter()
                    run[arm]()
                    reps[arm] = max(1, int(a.min_seconds / max(time.perf_counter() - t0, 1e-6)) + 1)
                if len(arms) == 2:
                    ra = dr["A"].to_host(np.uint8).reshape(batch, res)
                    rf = dr["F"].to_host(np.uint8).reshape(batch, res)
                    for j in range(batch):
                        if affine(curve, ra[j]) != affine(curve, rf[j]):
                            raise SystemExit(f"curve {curve} 2^{k} x {batch}: member {j} differs between the arms")
                name, mhz = device_line(lib, single, cfg_members[0])
                ms = {arm: [] for arm in arms}
                for _ in range(a.alternations):
                    for arm in arms:
                        t0 = time.perf_counter()
                        for _ in range(reps[arm]):
                            run[arm]()
                        ms[arm].append((time.perf_counter() - t0) / (reps[arm] * batch) * 1e3)
                rec = {"curve": curve, "log_n": k, "batch": batch, "window_bits": bits.value, "tables": tables.value, "group_log": group_log, "sequences": sequences,
                       "device": name, "sclk_mhz": mhz, "lib": "in-tree" if not a.lib else os.path.basename(os.path.dirname(ffi.LIB_PATH)) + "/" + os.path.basename(ffi.LIB_PATH),
                       "calls_per_repetition": reps, "per_member_ms": {arm: [round(v, 5) for v in ms[arm]] for arm in arms}}
                for arm in arms:
                    v = ms[arm]
                    rec[f"{arm}_min_med_max"] = [round(min(v), 5), round(statistics.median(v), 5), round(max(v), 5)]
                if "A" in arms and "F" in arms:
                    rec["F_over_A_median"] = round(statistics.median(ms["F"]) / statistics.median(ms["A"]), 4)
                base = baseline.get((curve, k, batch))
                if base and "F" in arms:
                    bmin, bmed, bmax = base["A_min_med_max"]
                    rec["baseline_A_min_med_max"] = base["A_min_med_max"]
                    rec["F_median_over_baseline_median"] = round(statistics.median(ms["F"]) / bmed, 4)
                    rec["F_slowest_beats_baseline_fastest"] = max(ms["F"]) < bmin
                    rec["F_median_within_baseline_spread"] = statistics.median(ms["F"]) <= bmed + (bmax - bmin)
                    if "A" in arms:
                        rec["A_median_within_baseline_spread"] = abs(statistics.median(ms["A"]) - bmed) <= max(bmax - bmin, max(ms["A"]) - min(ms["A"]))
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            finally:
                lib.panda_msm_unregister_bases(db.ptr)
                for d in [db, ds] + list(dr.values()):
                    d.free()
    finally:
        if out:
            out.close()
        gm.deinit()


if __name__ == "__main__":
    main()
