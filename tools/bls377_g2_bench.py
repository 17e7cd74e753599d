"""ms per call of the BLS12-377 G2 MSM (curve 6) beside BLS12-381 G2 (curve 4), in one process: 2^16, 2^18 and 2^20 points, plain
(unregistered bases) and with precomputed window tables, Jacobian and projective output.  Device-generated inputs; every
configuration is warmed up once and timed as the best of `reps` wall-clock calls (each call is synchronous).  A last line per
size and curve gives the per-phase device times of one tabled call (phase timers on): the share of the kernels behind k_accumulate.
Both fields are Fq2 over 14 limbs (four base products per Fq2 multiply); curve 6's u^2 = -5 adds a multiply by 5 and a carry pass to
the c0 of every product, its zero top limb of p saves multiply-adds.
usage: bls377_g2_bench.py [log_n,..] [reps]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gpu_util import NULL_STREAM, DeviceBuffer  # noqa: E402
from panda_amd import gpu_ffi as ffi  # noqa: E402
from panda_amd import gpu_manager as pgm  # noqa: E402

CURVES = {6: ("bls12_377_g2", 192, 288), 4: ("bls12_381_g2", 192, 288)}


def best_ms(fn, cfg, reps):
    ffi.check(fn(cfg), "msm")  # warm-up: arena, code objects
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        ffi.check(fn(cfg), "msm")
        dt = (time.perf_counter() - t) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def main():
    ks = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "16,18,20").split(",")]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    lib = ffi.load()
    gm = pgm.PandaGpuManager(0)
    names = [lib.panda_msm_phase_name(i).decode() for i in range(8)]
    rows = {}
    try:
        for k in ks:
            n = 1 << k
            for curve, (name, pt, res) in CURVES.items():
                fn = getattr(lib, f"panda_msm_execute_{name}")
                db, ds, dr = DeviceBuffer(n * pt), DeviceBuffer(n * 32), DeviceBuffer(res)
                ffi.check(lib.panda_gen_bases(curve, 0x6B + k, 0, n, db.ptr, NULL_STREAM), "gen")
                ffi.check(lib.panda_gen_scalars(curve, 0x6C + k, 0, n, ds.ptr, NULL_STREAM), "gen")
                for tabled in (False, True):
                    if tabled:
                        ffi.check(lib.panda_msm_precompute_bases(curve, db.ptr, k, 0, gm.exec_stream.raw), "precompute")
                    for coord in (pgm.JACOBIAN, pgm.PROJECTIVE):
                        cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, db.ptr, ds.ptr, dr.ptr, k, coord)
                        ms = best_ms(fn, cfg, reps)
                        rows[(k, curve, tabled, coord)] = ms
                        print(f"2^{k} curve {curve} {name:13s} {'tables' if tabled else 'plain ':6s} {'projective' if coord else 'jacobian  '} {ms:9.3f} ms", flush=True)
                lib.panda_msm_set_phase_timing(2)
                cfg = ffi.MSMConfiguration(gm.mem_pool, gm.exec_stream.raw, db.ptr, ds.ptr, dr.ptr, k, pgm.JACOBIAN)
                ffi.check(fn(cfg), "msm")
                ph = (C.c_float * 8)()
                lib.panda_msm_last_phase_ms(ph)
                lib.panda_msm_set_phase_timing(0)
                print(f"2^{k} curve {curve} phases (tables, timers on): " + " ".join(f"{nm}={v:.3f}" for nm, v in zip(names, ph)), flush=True)
                ffi.check(lib.panda_msm_unregister_bases(db.ptr), "unregister")
                for d in (db, ds, dr):
                    d.free()
            for tabled in (False, True):
                r = rows[(k, 6, tabled, pgm.JACOBIAN)] / rows[(k, 4, tabled, pgm.JACOBIAN)]
                print(f"2^{k} {'tables' if tabled else 'plain '} ratio curve 6 / curve 4 (jacobian): {r:.2f}x", flush=True)
    finally:
        gm.deinit()


if __name__ == "__main__":
    main()
