"""What panda_amd/gpu_manager.py asks of the library, call by call, and that every way out of a call gives back what the call took.

Each case runs one wrapper at a tiny shape against tests/fake_panda.py.  tests/golden/gpu_manager_calls.json holds, per case, the calls
of the success path and the PandaGpuError kind that a failure of each of them raises; it was recorded from the gpu_manager.py of the
commit before the wrappers moved onto one buffer scope (`python tests/test_gpu_manager_buffers.py --record` with that file's package
first on PYTHONPATH), so the trace and the kinds are the earlier code's.  The balance and the independence of the releases are what
the scope adds."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.append(ROOT)  # after PYTHONPATH: --record runs against whichever panda_amd comes first

from fake_panda import FakePanda  # noqa: E402
from panda_amd import gpu_ffi as ffi  # noqa: E402
from panda_amd import gpu_manager as m  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "gpu_manager_calls.json")
N, LOG_N = 8, 3


def fe(n=N, batch=None):
    return np.zeros((n, 8) if batch is None else (batch, n, 8), np.uint32)


def pts(n=N, nbytes=64):
    return np.zeros(n * nbytes, np.uint8)


def with_bases(log_n=LOG_N, register=False):
    def setup(gm):
        gm.add_cached_bases(pts(1 << log_n))
        if register:
            gm.register_cached_bases(0)
    return setup


def with_scalars(gm):
    gm.d_scalars.append(gm.init_msm_cached_scalars(fe()))
    gm.scalars_len.append(N * 32)


def with_both(gm):
    with_bases()(gm)
    with_scalars(gm)


def sparse(gm):
    return m.PandaSparseMatrix(gm, [0, 1, 2], [0, 1], fe(2), N)


def kzg(gm):
    return m.PandaKzgOpenAll(gm, pts(), fe(1))


TERMS = [(fe(1), [(0, 0), (1, 1)]), (fe(1), [])]
MLE_TERMS = [(fe(1), [0, 1])]


class Case:
    """run(gm, state) is the call under test, after setup(gm) -> state; `kept` is how many buffers the call documents as kept (negative:
    given back), `raises` the kind of a refusal that the call ends in, `scope_exit` whether its releases are those of a buffer scope"""

    def __init__(self, run, setup=None, kept=0, raises=None, scope_exit=True):
        self.run, self.setup, self.kept, self.raises, self.scope_exit = run, setup, kept, raises, scope_exit


CASES = {
    # MSM
    "msm": Case(lambda gm, _: m.panda_msm_bn254_gpu(gm, fe(), pts())),
    "msm_cached_bases": Case(lambda gm, _: m.panda_msm_bn254_gpu_with_cached_bases(gm, fe(), 0), with_bases()),
    "msm_cached_bases_2^18_plain": Case(lambda gm, _: m.panda_msm_bn254_gpu_with_cached_bases(gm, fe(1 << 18), 0), with_bases(18)),
    "msm_cached_bases_2^18_pipelined": Case(lambda gm, _: m.panda_msm_bn254_gpu_with_cached_bases(gm, fe(1 << 18), 0), with_bases(18, register=True)),
    "msm_cached_bases_batched_1": Case(lambda gm, _: m.panda_msm_bn254_gpu_with_cached_bases_batched(gm, [fe()], 0), with_bases()),
    "msm_cached_bases_batched_3": Case(lambda gm, _: m.panda_msm_bn254_gpu_with_cached_bases_batched(gm, [fe()] * 3, 0), with_bases()),
    "msm_batch_cached_bases": Case(lambda gm, _: m.panda_msm_gpu_batch_with_cached_bases(gm, [fe()] * 2, 0), with_bases()),
    "msm_cached_scalars": Case(lambda gm, _: m.panda_msm_bn254_gpu_with_cached_scalars(gm, 0, pts()), with_scalars),
    "msm_cached_scalars_bad_index": Case(lambda gm, _: m.panda_msm_bn254_gpu_with_cached_scalars(gm, 5, pts()), with_scalars, raises="BasesIndexErr"),
    "msm_cached_input": Case(lambda gm, _: m.panda_msm_bn254_gpu_with_cached_input(gm, 0, 0), with_both),
    "add_cached_bases": Case(lambda gm, _: gm.add_cached_bases(pts()), kept=1),
    "register_cached_bases": Case(lambda gm, _: gm.register_cached_bases(0), with_bases()),
    "precompute_cached_bases": Case(lambda gm, _: gm.precompute_cached_bases(0), with_bases()),
    "wait_h2d": Case(lambda gm, _: gm.wait_h2d()),
    "memory_alloc_and_copy": Case(lambda gm, _: m.memory_alloc_and_copy(gm, fe(), gm.h2d_stream), kept=1),
    # NTT
    "ntt": Case(lambda gm, _: m.panda_ntt_bn254_gpu(gm, fe(), LOG_N)),
    "ntt_v1": Case(lambda gm, _: m.panda_ntt_bn254_gpu_v1(gm, fe(), fe(1), LOG_N)),
    "ntt_coset": Case(lambda gm, _: m.panda_coset_ntt_bn254_gpu(gm, fe(), fe(1), fe(1), LOG_N)),
    "ntt_inverse": Case(lambda gm, _: m.panda_intt_bn254_gpu(gm, fe(), fe(1), LOG_N)),
    "ntt_bitrev": Case(lambda gm, _: m.panda_ntt_bn254_gpu_bitrev(gm, fe(), fe(1), LOG_N)),
    "ntt_bls12_381": Case(lambda gm, _: m.panda_ntt_bls12_381_gpu_v1(gm, fe(), fe(1), LOG_N)),
    "ntt_bls12_377": Case(lambda gm, _: m.panda_ntt_bls12_377_gpu_v1(gm, fe(), fe(1), LOG_N, inverse=True)),
    "ntt_bls12_377_bitrev": Case(lambda gm, _: m.panda_ntt_bls12_377_gpu_bitrev(gm, fe(), fe(1), LOG_N)),
    "ntt_bls12_377_coset": Case(lambda gm, _: m.panda_coset_ntt_bls12_377_gpu(gm, fe(), fe(1), fe(1), LOG_N, inverse=True)),
    "ntt_batch": Case(lambda gm, _: m.panda_ntt_gpu_batch(gm, [fe(), fe()], fe(1), LOG_N)),
    "ntt_batch_coset": Case(lambda gm, _: m.panda_ntt_gpu_batch(gm, [fe()] * 3, fe(1), LOG_N, kind=ffi.NTT_COSET, shift=fe(1))),
    "ntt_lde": Case(lambda gm, _: m.panda_ntt_gpu_lde(gm, [fe(), fe()], fe(1), LOG_N, 1, fe(1))),
    # scalar-field columns
    "poly_evaluate": Case(lambda gm, _: m.panda_poly_gpu_evaluate(gm, [fe(), fe()], fe(2))),
    "poly_divide": Case(lambda gm, _: m.panda_poly_gpu_divide(gm, [fe(), fe()], fe(1))),
    "poly_evaluate_lagrange": Case(lambda gm, _: m.panda_poly_gpu_evaluate_lagrange(gm, [fe(), fe()], fe(1), fe(2))),
    "poly_evaluate_lagrange_shift": Case(lambda gm, _: m.panda_poly_gpu_evaluate_lagrange(gm, [fe(), fe()], fe(1), fe(2), shift=fe(1))),
    "poly_evaluate_lagrange_not_2^k": Case(lambda gm, _: m.panda_poly_gpu_evaluate_lagrange(gm, [fe(6)], fe(1), fe(2)), raises="SchedulingErr"),
    "poly_divide_lagrange": Case(lambda gm, _: m.panda_poly_gpu_divide_lagrange(gm, [fe(), fe()], fe(1), fe(1))),
    "poly_divide_lagrange_not_2^k": Case(lambda gm, _: m.panda_poly_gpu_divide_lagrange(gm, [fe(6)], fe(1), fe(1)), raises="SchedulingErr"),
    "batch_inverse": Case(lambda gm, _: m.panda_field_gpu_batch_inverse(gm, [fe(), fe()])),
    "grand_product": Case(lambda gm, _: m.panda_poly_gpu_grand_product(gm, [fe(), fe()], None)),
    "grand_product_dens": Case(lambda gm, _: m.panda_poly_gpu_grand_product(gm, [fe(), fe()], [fe(), fe()])),
    "grand_product_dens_other_length": Case(lambda gm, _: m.panda_poly_gpu_grand_product(gm, [fe(), fe()], [fe(4), fe(4)]), raises="SchedulingErr"),
    "running_sum": Case(lambda gm, _: m.panda_poly_gpu_running_sum(gm, [fe(), fe()])),
    "lookup_multiplicities": Case(lambda gm, _: m.panda_lookup_gpu_multiplicities(gm, fe(4), [fe(), fe()])),
    "sum_of_products": Case(lambda gm, _: m.panda_poly_gpu_sum_of_products(gm, [fe(), fe()], TERMS)),
    "sum_of_products_batch_scales": Case(lambda gm, _: m.panda_poly_gpu_sum_of_products(gm, [fe(N, 2), fe(N, 2)], TERMS, scales=fe(2),
                                                                                          scale_mode=ffi.SOP_SCALE_CYCLIC)),
    "eq_table": Case(lambda gm, _: m.panda_mle_gpu_eq_table(gm, fe(LOG_N))),
    "eq_table_k0": Case(lambda gm, _: m.panda_mle_gpu_eq_table(gm, fe(0))),
    "sumcheck": Case(lambda gm, _: m.panda_sumcheck_gpu_run(gm, [fe(), fe()], MLE_TERMS, 2, fe(LOG_N))),
    "sumcheck_fused": Case(lambda gm, _: m.panda_sumcheck_gpu_run(gm, [fe(), fe()], MLE_TERMS, 2, fe(LOG_N), fused=True)),
    "sparse_construct": Case(lambda gm, _: sparse(gm), kept=3),
    "sparse_construct_empty": Case(lambda gm, _: m.PandaSparseMatrix(gm, [0, 0], [], fe(0), N), kept=1),
    "sparse_matvec": Case(lambda gm, a: a.matvec(fe()), sparse),
    "sparse_matvec_batch": Case(lambda gm, a: a.matvec(fe(N, 2)), sparse),
    "sparse_free": Case(lambda gm, a: a.free(), sparse, kept=-3, scope_exit=False),
    "sparse_one_call": Case(lambda gm, _: m.panda_sparse_gpu_matvec(gm, [0, 1, 2], [0, 1], fe(2), fe(), N), scope_exit=False),
    # points
    "ec_ntt": Case(lambda gm, _: m.panda_ec_ntt_gpu(gm, pts(), fe(1))),
    "points_to_affine": Case(lambda gm, _: m.panda_points_gpu_to_affine(gm, pts(2, 96))),
    "points_mul_each": Case(lambda gm, _: m.panda_points_gpu_scalar_mul(gm, pts(2), fe(2))),
    "points_mul_one": Case(lambda gm, _: m.panda_points_gpu_scalar_mul(gm, pts(2), fe(1), mode=ffi.POINTS_MUL_ONE)),
    "points_mul_powers": Case(lambda gm, _: m.panda_points_gpu_scalar_mul(gm, pts(2), fe(2), mode=ffi.POINTS_MUL_POWERS)),
    "points_mul_each_addend": Case(lambda gm, _: m.panda_points_gpu_scalar_mul(gm, pts(2), fe(2), addend=pts(2))),
    "kzg_construct": Case(lambda gm, _: kzg(gm), kept=3),
    "kzg_open": Case(lambda gm, k: k.open(fe()), kzg),
    "kzg_close": Case(lambda gm, k: k.close(), kzg, kept=-3, scope_exit=False),
}


class Run:
    """one run of a case on a fresh fake and manager: the fake, what was live before the call, and the kind the call raised (or None)"""

    def __init__(self, case, fail_at=None, fail_release=None):
        self.fake = fake = FakePanda()
        load, ffi.load = ffi.load, lambda: fake
        try:
            gm = m.PandaGpuManager(0)
            fake.streams = {s.raw.handle: label for label, s in (("default", gm.default_stream), ("h2d", gm.h2d_stream), ("d2h", gm.d2h_stream),
                                                                    ("exec", gm.exec_stream))}
            state = case.setup(gm) if case.setup else None
            self.before = set(fake.live)
            fake.begin(fail_at, fail_release)
            try:
                case.run(gm, state)
                self.kind = None
            except m.PandaGpuError as e:
                self.kind = e.kind
        finally:
            ffi.load = load


def record():
    out = {}
    for name, case in CASES.items():
        run = Run(case)
        assert run.kind == case.raises, (name, run.kind)
        kinds = [Run(case, fail_at=k + 1).kind for k in range(len(run.fake.calls))]
        out[name] = {"calls": run.fake.calls, "releases": run.fake.releases, "kinds": kinds}
    with open(GOLDEN, "w") as f:  # one call a line
        f.write("{\n" + ",\n".join(
            f"{json.dumps(name)}: {{\n" + ",\n".join(
                f' {json.dumps(key)}: [\n' + ",\n".join("  " + json.dumps(x) for x in rec[key]) + "\n ]" for key in ("calls", "releases", "kinds")) + "\n}"
            for name, rec in out.items()) + "\n}\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_success_path_makes_the_recorded_calls(name, golden):
    run = Run(CASES[name])
    assert run.kind == CASES[name].raises
    assert run.fake.calls == golden[name]["calls"]
    if not CASES[name].raises:  # a refusal after staging left the staged buffer allocated when the file was recorded
        assert sorted(map(json.dumps, run.fake.releases)) == sorted(map(json.dumps, golden[name]["releases"]))


@pytest.mark.parametrize("name", CASES)
def test_each_failing_call_raises_the_recorded_kind(name, golden):
    kinds = golden[name]["kinds"]
    assert len(kinds) == len(golden[name]["calls"])
    assert [Run(CASES[name], fail_at=k + 1).kind for k in range(len(kinds))] == kinds


@pytest.mark.parametrize("name", CASES)
def test_every_way_out_gives_back_what_the_call_took(name, golden):
    case = CASES[name]
    run = Run(case)
    live = set(run.fake.live)
    assert (len(live - run.before), len(run.before - live)) == (max(case.kept, 0), max(-case.kept, 0))
    if case.raises:
        assert live == run.before
    for k in range(len(golden[name]["calls"])):
        failed = Run(case, fail_at=k + 1)
        left = sorted(v for key, v in failed.fake.live.items() if key not in failed.before)
        assert set(failed.fake.live) == failed.before, f"call {k + 1} ({golden[name]['calls'][k][0]}) failing leaves {left}"


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.scope_exit])
def test_releases_are_independent(name):
    case = CASES[name]
    releases = Run(case).fake.releases
    for j in range(len(releases)):
        run = Run(case, fail_release=j + 1)
        assert run.kind == (case.raises or "CreateContextError")
        assert sorted(map(json.dumps, run.fake.releases)) == sorted(map(json.dumps, releases))  # all attempted, each once
        live = set(run.fake.live)
        assert run.before <= live and len(live - run.before) == case.kept + 1  # only the one whose release failed stays


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_gpu_manager_buffers.py --record   (writes tests/golden/gpu_manager_calls.json from the panda_amd that PYTHONPATH puts first)")
    record()
