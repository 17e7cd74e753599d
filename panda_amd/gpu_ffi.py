"""ctypes binding of the C ABI in include/panda_interface.h.

Python counterpart of the reference's Rust `gpu_ffi` layer (src/gpu_ffi/binding.rs:3-115 for the
extern block, src/gpu_ffi/common.rs:5-208 for the repr(C) structs and the error enum): same symbol
names, same by-value handle and configuration structs, same "non-zero means failure" convention.
The library is the in-tree HIP build (panda_amd/csrc/libpanda-cuda.so); there is no fallback:
loading fails loudly if it has not been built.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpanda-cuda.so")


class PandaGpuError(RuntimeError):
    """Mirrors enum PandaGpuError (gpu_ffi/common.rs:5-38); `kind` carries the variant name."""

    def __init__(self, kind: str, code: int = 0):
        super().__init__(f"{kind} (panda_error={code})")
        self.kind, self.code = kind, code


class PandaStream(C.Structure):  # gpu_ffi/common.rs:40-44
    _fields_ = [("handle", C.c_void_p)]


class PandaEvent(C.Structure):  # gpu_ffi/common.rs:89-93
    _fields_ = [("handle", C.c_void_p)]


class PandaMemPool(C.Structure):  # gpu_ffi/common.rs:134-138
    _fields_ = [("handle", C.c_void_p)]


JACOBIAN, PROJECTIVE = 0, 1  # PandaMSMResultCoordinateType, gpu_ffi/common.rs:160-166


class MSMConfiguration(C.Structure):  # gpu_ffi/common.rs:168-185, panda_interface.cuh:70-79
    _fields_ = [("mem_pool", PandaMemPool), ("stream", PandaStream), ("bases", C.c_void_p), ("scalars", C.c_void_p),
                ("results", C.c_void_p), ("log_scalars_count", C.c_uint), ("msm_result_coordinate_type", C.c_int)]


class NTTConfiguration(C.Structure):  # gpu_ffi/common.rs:187-196
    _fields_ = [("mem_pool", PandaMemPool), ("stream", PandaStream), ("d_src", C.c_void_p), ("d_dst", C.c_void_p),
                ("log_n", C.c_uint), ("flag", C.POINTER(C.c_uint))]


class NttconfigurationV1(C.Structure):  # gpu_ffi/common.rs:198-208
    _fields_ = [("mem_pool", PandaMemPool), ("stream", PandaStream), ("d_src", C.c_void_p), ("d_dst", C.c_void_p),
                ("omega", C.c_void_p), ("log_n", C.c_uint), ("flag", C.POINTER(C.c_uint))]


class PandaMultiGpu(C.Structure):  # additive: include/panda_interface.h panda_multi_gpu (one process, one worker thread + RCCL communicator per device)
    _fields_ = [("handle", C.c_void_p)]


MULTI_RCCL, MULTI_LOOPBACK = 0, 1
NTT_MAX_BATCH = 4096  # PANDA_NTT_MAX_BATCH
# `kind` of panda_ntt_execute_batch: which single call a member runs as (PANDA_NTT_FORWARD ...)
NTT_FORWARD, NTT_INVERSE, NTT_BITREV_OUT, NTT_INVERSE_BITREV_IN, NTT_COSET, NTT_COSET_INVERSE = range(6)
# `order` of panda_ntt_execute_lde (PANDA_NTT_LDE_COSET_MAJOR, PANDA_NTT_LDE_NATURAL) and its largest log2 of the blow-up
NTT_LDE_COSET_MAJOR, NTT_LDE_NATURAL = 0, 1
NTT_LDE_MAX_LOG_BLOWUP = 4  # PANDA_NTT_LDE_MAX_LOG_BLOWUP
POLY_MAX_POINTS = 8  # PANDA_POLY_MAX_POINTS
# `order` of panda_poly_evaluate_lagrange / panda_poly_divide_linear_lagrange (PANDA_DOMAIN_NATURAL, PANDA_DOMAIN_BITREV)
DOMAIN_NATURAL, DOMAIN_BITREV = 0, 1
# panda_poly_sum_of_products: the caps of an expression (PANDA_SOP_MAX_*) and its scale modes (PANDA_SOP_SCALE_*)
SOP_MAX_COLUMNS, SOP_MAX_TERMS, SOP_MAX_FACTORS, SOP_MAX_SCALES = 32, 64, 256, 16
SOP_SCALE_NONE, SOP_SCALE_PER_VECTOR, SOP_SCALE_CYCLIC = 0, 1, 2
LOOKUP_MAX_COLUMNS = 32  # PANDA_LOOKUP_MAX_COLUMNS
# panda_sumcheck_round / panda_mle_fold: the binding orders (PANDA_MLE_BIND_*) and the most evaluation points of a round polynomial
MLE_BIND_LOW, MLE_BIND_HIGH = 0, 1
SUMCHECK_MAX_EVALS = 8  # PANDA_SUMCHECK_MAX_EVALS
# `direction` of panda_ec_ntt (PANDA_EC_NTT_FORWARD, PANDA_EC_NTT_INVERSE) and its largest log2 of the size
EC_NTT_FORWARD, EC_NTT_INVERSE = 0, 1
EC_NTT_MAX_LOG_N = 26  # PANDA_EC_NTT_MAX_LOG_N
# `mode` of panda_points_scalar_mul (PANDA_POINTS_MUL_*) and the largest log2 of a panda_kzg_open_all domain
POINTS_MUL_EACH, POINTS_MUL_ONE, POINTS_MUL_POWERS = 0, 1, 2
KZG_OPEN_ALL_MAX_LOG_N = 25  # PANDA_KZG_OPEN_ALL_MAX_LOG_N
POSEIDON_MAX_WIDTH = 5  # PANDA_POSEIDON_MAX_WIDTH
CLOCK_WORDS, CLOCK_STAMP_BYTES = 12, 32768  # PANDA_CLOCK_WORDS, PANDA_CLOCK_STAMP_BYTES


class NttSlabConfiguration(C.Structure):  # additive: include/panda_interface.h panda_ntt_slab_configuration
    _fields_ = [("stream", PandaStream), ("d_slab", C.c_void_p), ("d_scratch", C.c_void_p), ("omega", C.c_void_p),
                ("log_n", C.c_uint), ("log_ranks", C.c_uint), ("rank", C.c_uint), ("flag", C.POINTER(C.c_uint))]


class SopFactor(C.Structure):  # additive: include/panda_interface.h panda_sop_factor
    _fields_ = [("column", C.c_uint32), ("rotation", C.c_int32)]


class SopExpression(C.Structure):  # additive: include/panda_interface.h panda_sop_expression; every pointer is a HOST pointer
    _fields_ = [("columns", C.POINTER(C.c_void_p)), ("coeffs", C.c_void_p), ("degrees", C.POINTER(C.c_uint)), ("factors", C.POINTER(SopFactor)),
                ("scales", C.c_void_p), ("n_columns", C.c_uint), ("n_terms", C.c_uint), ("n_scales", C.c_uint), ("scale_mode", C.c_uint)]


class CsrMatrix(C.Structure):  # additive: include/panda_interface.h panda_csr_matrix; every pointer is a DEVICE pointer
    _fields_ = [("d_row_ptr", C.c_void_p), ("d_col", C.c_void_p), ("d_values", C.c_void_p), ("n_rows", C.c_uint64), ("n_cols", C.c_uint64),
                ("nnz", C.c_uint64)]


class PoseidonParams(C.Structure):  # additive: include/panda_interface.h panda_poseidon_params; both pointers are HOST pointers
    _fields_ = [("width", C.c_uint), ("alpha", C.c_uint), ("full_rounds", C.c_uint), ("partial_rounds", C.c_uint), ("round_constants", C.c_void_p),
                ("mds", C.c_void_p)]


class PandaPoseidon(C.Structure):  # additive: include/panda_interface.h panda_poseidon (a parameter set and its device table)
    _fields_ = [("handle", C.c_void_p)]


# every symbol include/panda_interface.h declares; tests assert the library exports each one
REFERENCE_SYMBOLS = [
    "panda_get_device_number", "panda_get_device", "panda_set_device", "panda_stream_create", "panda_stream_wait_event",
    "panda_stream_sync", "panda_stream_destroy", "panda_launch_host_fn", "panda_event_create", "panda_event_record",
    "panda_event_sync", "panda_event_query", "panda_event_destroy", "panda_mem_get_info", "panda_malloc", "panda_malloc_host",
    "panda_free", "panda_free_host", "panda_host_register", "panda_host_unregister", "panda_memcpy", "panda_memcpy_async",
    "panda_memset", "panda_memset_async", "panda_mem_pool_create", "panda_mem_pool_destroy", "panda_malloc_from_pool_async",
    "panda_free_async", "panda_msm_setup_bn254", "panda_msm_execute_bn254", "panda_msm_execute_bn254_host", "panda_msm_tear_down",
    "panda_ntt_setup_bn254", "panda_ntt_execute_bn254", "panda_ntt_tear_down", "panda_ntt_execute_bn254_v1",
]
RUST_ONLY_SYMBOLS = ["panda_stream_synchronize", "panda_stream_query", "panda_device_enable_peer_access", "panda_device_disable_peer_access"]
ADDITIVE_SYMBOLS = [
    "panda_msm_register_bases", "panda_msm_unregister_bases", "panda_msm_execute_from_host", "panda_msm_precompute_bases", "panda_msm_registered_info", "panda_msm_set_chunk_entries", "panda_msm_set_overlap", "panda_msm_set_accumulate_variant", "panda_msm_set_wide_merge", "panda_msm_set_reduce_group", "panda_msm_plain_window_plan", "panda_msm_verify_registered", "panda_msm_set_paranoid", "panda_msm_set_phase_timing", "panda_msm_setup_bls12_377", "panda_msm_execute_bls12_377", "panda_msm_execute_bls12_377_host", "panda_msm_set_window_bits", "panda_msm_execute_batch", "panda_msm_batch_plan",
    "panda_msm_last_phase_ms", "panda_msm_phase_name", "panda_ntt_last_device_ms", "panda_ntt_pass_plan", "panda_ntt_set_streamed_tables", "panda_ntt_execute_bn254_inverse", "panda_ntt_execute_bls12_377_v1", "panda_ntt_execute_bls12_377_inverse", "panda_msm_combine_bn254",
    "panda_msm_combine_bls12_377", "panda_msm_setup_bn254_g2", "panda_msm_execute_bn254_g2", "panda_msm_execute_bn254_g2_host", "panda_msm_combine_bn254_g2", "panda_msm_setup_bls12_381", "panda_msm_execute_bls12_381", "panda_msm_execute_bls12_381_host", "panda_msm_combine_bls12_381",
    "panda_ntt_execute_bls12_381_v1", "panda_ntt_execute_bls12_381_inverse", "panda_ntt_execute_bn254_coset", "panda_ntt_execute_bn254_coset_inverse", "panda_ntt_execute_bn254_bitrev_out", "panda_ntt_execute_bn254_inverse_bitrev_in", "panda_ntt_slab_step1_bn254", "panda_ntt_slab_step2_bn254", "panda_ntt_slab_step1_bn254_enqueue", "panda_ntt_slab_step2_bn254_enqueue", "panda_ntt_slab_inverse_step1_bn254_enqueue", "panda_ntt_slab_inverse_step2_bn254_enqueue", "panda_gen_scalars", "panda_gen_bases",
    "panda_debug_field_op", "panda_debug_curve_op", "panda_debug_fe_internal", "panda_debug_xyzz_internal", "panda_debug_scratch_fill", "panda_version",
    "panda_ntt_table_builds", "panda_msm_set_chunk_first", "panda_set_clock_stamps", "panda_msm_last_clock", "panda_ntt_last_clock", "panda_clock_stamp", "panda_clock_delta",
    "panda_multi_gpu_create", "panda_multi_gpu_destroy", "panda_multi_gpu_device_count", "panda_msm_execute_bn254_multi", "panda_msm_execute_bls12_377_multi",
    "panda_msm_execute_bn254_from_host_multi", "panda_msm_execute_bls12_377_from_host_multi",
    "panda_msm_execute_bls12_381_multi", "panda_msm_execute_bn254_g2_multi", "panda_msm_execute_bls12_381_from_host_multi", "panda_msm_execute_bn254_g2_from_host_multi",
    "panda_ntt_execute_bn254_multi", "panda_ntt_execute_bn254_inverse_multi", "panda_ntt_execute_bn254_multi_batch", "panda_ntt_execute_bn254_inverse_multi_batch", "panda_multi_gpu_last_phase_ms",
    "panda_ntt_execute_bls12_377_bitrev_out", "panda_ntt_execute_bls12_377_inverse_bitrev_in", "panda_ntt_execute_bls12_377_coset", "panda_ntt_execute_bls12_377_coset_inverse",
    "panda_ntt_slab_step1_bls12_377_enqueue", "panda_ntt_slab_step2_bls12_377_enqueue", "panda_ntt_slab_inverse_step1_bls12_377_enqueue", "panda_ntt_slab_inverse_step2_bls12_377_enqueue",
    "panda_ntt_execute_bls12_377_multi", "panda_ntt_execute_bls12_377_inverse_multi", "panda_ntt_execute_bls12_377_multi_batch", "panda_ntt_execute_bls12_377_inverse_multi_batch",
    "panda_ntt_execute_bls12_381_bitrev_out", "panda_ntt_execute_bls12_381_inverse_bitrev_in", "panda_ntt_execute_bls12_381_coset", "panda_ntt_execute_bls12_381_coset_inverse", "panda_ntt_slab_step1_bls12_381_enqueue", "panda_ntt_slab_step2_bls12_381_enqueue", "panda_ntt_slab_inverse_step1_bls12_381_enqueue", "panda_ntt_slab_inverse_step2_bls12_381_enqueue", "panda_ntt_execute_bls12_381_multi", "panda_ntt_execute_bls12_381_inverse_multi", "panda_ntt_execute_bls12_381_multi_batch", "panda_ntt_execute_bls12_381_inverse_multi_batch",
    "panda_msm_setup_bls12_381_g2", "panda_msm_execute_bls12_381_g2", "panda_msm_execute_bls12_381_g2_host", "panda_msm_combine_bls12_381_g2",
    "panda_msm_execute_bls12_381_g2_multi", "panda_msm_execute_bls12_381_g2_from_host_multi",
    "panda_msm_setup_bls12_377_g2", "panda_msm_execute_bls12_377_g2", "panda_msm_execute_bls12_377_g2_host", "panda_msm_combine_bls12_377_g2",
    "panda_msm_execute_bls12_377_g2_multi", "panda_msm_execute_bls12_377_g2_from_host_multi",
    "panda_ntt_execute_batch", "panda_ntt_batch_plan",
    "panda_ntt_execute_lde", "panda_ntt_lde_plan",
    "panda_poly_evaluate", "panda_poly_divide_linear", "panda_poly_plan",
    "panda_poly_evaluate_lagrange", "panda_poly_divide_linear_lagrange", "panda_poly_lagrange_plan",
    "panda_field_batch_inverse", "panda_poly_grand_product", "panda_poly_product_plan",
    "panda_poly_sum_of_products", "panda_poly_sum_of_products_plan",
    "panda_lookup_multiplicities", "panda_lookup_plan", "panda_lookup_home_slot", "panda_poly_running_sum", "panda_poly_running_sum_plan",
    "panda_sumcheck_round", "panda_mle_fold", "panda_mle_eq_table", "panda_sumcheck_plan",
    "panda_sparse_matvec", "panda_sparse_check", "panda_sparse_plan",
    "panda_ec_ntt", "panda_ec_ntt_plan", "panda_points_to_affine", "panda_points_to_affine_plan",
    "panda_points_scalar_mul", "panda_points_scalar_mul_plan", "panda_kzg_open_all_setup", "panda_kzg_open_all", "panda_kzg_open_all_plan",
    "panda_poseidon_create", "panda_poseidon_destroy", "panda_poseidon_permute", "panda_poseidon_hash", "panda_poseidon_merkle_tree", "panda_poseidon_plan",
]
ALL_SYMBOLS = REFERENCE_SYMBOLS + RUST_ONLY_SYMBOLS + ADDITIVE_SYMBOLS

_lib = None


def load() -> C.CDLL:
    """dlopen the HIP library.  torch, when installed, is imported first so that the process ends up
    with ONE libamdhip64 (torch bundles its own copy under the same SONAME)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C panda_amd/csrc).  There is no CPU fallback for the product path.")
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing, not a requirement of the library
        pass
    lib = C.CDLL(LIB_PATH)
    u, sz, vp = C.c_uint, C.c_size_t, C.c_void_p
    sig = {
        "panda_get_device_number": [C.POINTER(C.c_int)], "panda_get_device": [C.POINTER(C.c_int)], "panda_set_device": [C.c_int],
        "panda_stream_create": [C.POINTER(PandaStream), C.c_bool], "panda_stream_wait_event": [PandaStream, PandaEvent],
        "panda_stream_sync": [PandaStream], "panda_stream_synchronize": [PandaStream], "panda_stream_query": [PandaStream],
        "panda_stream_destroy": [PandaStream], "panda_launch_host_fn": [PandaStream, vp, vp],
        "panda_event_create": [C.POINTER(PandaEvent), C.c_bool, C.c_bool], "panda_event_record": [PandaEvent, PandaStream],
        "panda_event_sync": [PandaEvent], "panda_event_query": [PandaEvent], "panda_event_destroy": [PandaEvent],
        "panda_mem_get_info": [C.POINTER(sz), C.POINTER(sz)], "panda_malloc": [C.POINTER(vp), sz], "panda_malloc_host": [C.POINTER(vp), sz],
        "panda_free": [vp], "panda_free_host": [vp], "panda_host_register": [vp, sz], "panda_host_unregister": [vp],
        "panda_memcpy": [vp, vp, sz], "panda_memcpy_async": [vp, vp, sz, PandaStream], "panda_memset": [vp, C.c_int, sz],
        "panda_memset_async": [vp, C.c_int, sz, PandaStream], "panda_mem_pool_create": [C.POINTER(PandaMemPool), C.c_int],
        "panda_mem_pool_destroy": [PandaMemPool], "panda_malloc_from_pool_async": [C.POINTER(vp), sz, PandaMemPool, PandaStream],
        "panda_free_async": [vp, PandaStream], "panda_msm_setup_bn254": [], "panda_msm_execute_bn254": [MSMConfiguration],
        "panda_msm_execute_bn254_host": [MSMConfiguration], "panda_msm_tear_down": [], "panda_ntt_setup_bn254": [vp],
        "panda_ntt_execute_bn254": [NTTConfiguration], "panda_ntt_tear_down": [], "panda_ntt_execute_bn254_v1": [NttconfigurationV1],
        "panda_device_enable_peer_access": [C.c_int], "panda_device_disable_peer_access": [C.c_int],
        "panda_msm_execute_from_host": [u, MSMConfiguration, vp, u, PandaStream],
        "panda_msm_execute_batch": [u, MSMConfiguration, u], "panda_msm_batch_plan": [u, u, u, u, C.POINTER(u), C.POINTER(u)],
        "panda_ntt_execute_batch": [u, u, NttconfigurationV1, u, vp], "panda_ntt_batch_plan": [u, u, u, C.POINTER(u), C.POINTER(u)],
        "panda_ntt_execute_lde": [u, NttconfigurationV1, vp, u, u, vp, u], "panda_ntt_lde_plan": [u, u, u, u, C.POINTER(u), C.POINTER(u)],
        "panda_poly_evaluate": [u, vp, C.c_uint64, u, vp, u, vp, PandaStream], "panda_poly_divide_linear": [u, vp, vp, C.c_uint64, u, vp, vp, PandaStream],
        "panda_poly_plan": [C.c_uint64, u, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)],
        "panda_poly_evaluate_lagrange": [u, vp, u, u, vp, vp, u, vp, u, vp, PandaStream],
        "panda_poly_divide_linear_lagrange": [u, vp, vp, u, u, vp, vp, u, vp, vp, PandaStream],
        "panda_poly_lagrange_plan": [u, u, u, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)],
        "panda_field_batch_inverse": [u, vp, vp, C.c_uint64, PandaStream], "panda_poly_grand_product": [u, vp, vp, vp, C.c_uint64, u, vp, PandaStream],
        "panda_poly_product_plan": [C.c_uint64, u, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)],
        "panda_poly_sum_of_products": [u, C.POINTER(SopExpression), vp, C.c_uint64, u, PandaStream],
        "panda_poly_sum_of_products_plan": [C.c_uint64, u, C.POINTER(u), C.POINTER(u)],
        "panda_lookup_multiplicities": [u, vp, C.c_uint64, C.POINTER(vp), u, C.c_uint64, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), PandaStream],
        "panda_lookup_plan": [C.c_uint64, u, C.c_uint64, C.POINTER(u), C.POINTER(sz), C.POINTER(u)],
        "panda_lookup_home_slot": [u, vp, u, C.POINTER(C.c_uint64)],
        "panda_poly_running_sum": [u, vp, vp, C.c_uint64, u, vp, PandaStream],
        "panda_poly_running_sum_plan": [C.c_uint64, u, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)],
        "panda_sumcheck_round": [u, C.POINTER(SopExpression), u, u, u, vp, C.POINTER(vp), vp, PandaStream],
        "panda_mle_fold": [u, C.POINTER(vp), C.POINTER(vp), u, u, u, vp, PandaStream],
        "panda_mle_eq_table": [u, vp, u, vp, PandaStream],
        "panda_sumcheck_plan": [u, u, u, C.POINTER(u), C.POINTER(u), C.POINTER(u)],
        "panda_sparse_matvec": [u, C.POINTER(CsrMatrix), vp, vp, u, PandaStream],
        "panda_sparse_check": [u, C.POINTER(CsrMatrix), C.POINTER(u), C.POINTER(C.c_uint64), PandaStream],
        "panda_sparse_plan": [C.c_uint64, C.c_uint64, C.c_uint64, u, C.POINTER(u), C.POINTER(u), C.POINTER(sz), C.POINTER(u)],
        "panda_poseidon_create": [u, C.POINTER(PoseidonParams), C.POINTER(PandaPoseidon)], "panda_poseidon_destroy": [PandaPoseidon],
        "panda_poseidon_permute": [PandaPoseidon, vp, vp, C.c_uint64, PandaStream],
        "panda_poseidon_hash": [PandaPoseidon, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, PandaStream],
        "panda_poseidon_merkle_tree": [PandaPoseidon, vp, u, vp, vp, vp, PandaStream],
        "panda_poseidon_plan": [u, u, C.POINTER(u), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(u), C.POINTER(u)],
        "panda_ec_ntt": [u, vp, vp, u, u, vp, PandaStream], "panda_ec_ntt_plan": [u, u, u, C.POINTER(u), C.POINTER(sz), C.POINTER(u)],
        "panda_points_to_affine": [u, vp, C.c_int, vp, C.c_uint64, PandaStream], "panda_points_to_affine_plan": [C.c_uint64, C.POINTER(u), C.POINTER(u)],
        "panda_points_scalar_mul": [u, u, vp, vp, vp, vp, vp, C.c_uint64, PandaStream], "panda_points_scalar_mul_plan": [u, u, C.c_uint64, C.POINTER(u), C.POINTER(sz)],
        "panda_kzg_open_all_setup": [u, vp, u, vp, vp, PandaStream], "panda_kzg_open_all": [u, vp, vp, u, vp, vp, sz, vp, PandaStream],
        "panda_kzg_open_all_plan": [u, u, C.POINTER(sz), C.POINTER(u)],
        "panda_msm_register_bases": [u, vp, u, PandaStream], "panda_msm_unregister_bases": [vp], "panda_msm_precompute_bases": [u, vp, u, u, PandaStream],
        "panda_msm_registered_info": [vp, C.POINTER(u), C.POINTER(u), C.POINTER(sz)], "panda_msm_set_chunk_entries": [u], "panda_msm_set_overlap": [u, u], "panda_msm_set_accumulate_variant": [u], "panda_msm_set_wide_merge": [u], "panda_msm_set_reduce_group": [u], "panda_msm_plain_window_plan": [u, u, C.POINTER(u), C.POINTER(u)], "panda_msm_verify_registered": [vp, PandaStream], "panda_msm_set_paranoid": [u], "panda_msm_set_phase_timing": [u], "panda_msm_setup_bls12_377": [], "panda_msm_execute_bls12_377": [MSMConfiguration], "panda_msm_execute_bls12_377_host": [MSMConfiguration],
        "panda_msm_set_window_bits": [u], "panda_msm_last_phase_ms": [C.POINTER(C.c_float)], "panda_ntt_last_device_ms": [C.POINTER(C.c_float)], "panda_ntt_pass_plan": [u, C.POINTER(C.c_uint), C.POINTER(C.c_uint)], "panda_ntt_set_streamed_tables": [u], "panda_ntt_execute_bn254_inverse": [NttconfigurationV1], "panda_ntt_execute_bls12_377_v1": [NttconfigurationV1], "panda_ntt_execute_bls12_377_inverse": [NttconfigurationV1],
        "panda_msm_combine_bn254": [vp, u, C.c_int, vp], "panda_msm_combine_bls12_377": [vp, u, C.c_int, vp], "panda_msm_combine_bls12_381": [vp, u, C.c_int, vp],
        "panda_msm_setup_bn254_g2": [], "panda_msm_execute_bn254_g2": [MSMConfiguration], "panda_msm_execute_bn254_g2_host": [MSMConfiguration],
        "panda_msm_combine_bn254_g2": [vp, u, C.c_int, vp],
        "panda_msm_setup_bls12_381_g2": [], "panda_msm_execute_bls12_381_g2": [MSMConfiguration], "panda_msm_execute_bls12_381_g2_host": [MSMConfiguration],
        "panda_msm_combine_bls12_381_g2": [vp, u, C.c_int, vp],
        "panda_msm_execute_bls12_381_g2_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), vp],
        "panda_msm_execute_bls12_381_g2_from_host_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), C.POINTER(vp), u, vp],
        "panda_msm_setup_bls12_377_g2": [], "panda_msm_execute_bls12_377_g2": [MSMConfiguration], "panda_msm_execute_bls12_377_g2_host": [MSMConfiguration],
        "panda_msm_combine_bls12_377_g2": [vp, u, C.c_int, vp],
        "panda_msm_execute_bls12_377_g2_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), vp],
        "panda_msm_execute_bls12_377_g2_from_host_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), C.POINTER(vp), u, vp],
        "panda_msm_setup_bls12_381": [], "panda_msm_execute_bls12_381": [MSMConfiguration], "panda_msm_execute_bls12_381_host": [MSMConfiguration],
        "panda_ntt_execute_bls12_381_v1": [NttconfigurationV1], "panda_ntt_execute_bls12_381_inverse": [NttconfigurationV1],
        "panda_ntt_execute_bn254_bitrev_out": [NttconfigurationV1], "panda_ntt_execute_bn254_inverse_bitrev_in": [NttconfigurationV1],
        "panda_ntt_execute_bn254_coset": [NttconfigurationV1, vp], "panda_ntt_execute_bn254_coset_inverse": [NttconfigurationV1, vp],
        "panda_ntt_slab_step1_bn254": [NttSlabConfiguration], "panda_ntt_slab_step2_bn254": [NttSlabConfiguration],
        "panda_ntt_slab_step1_bn254_enqueue": [NttSlabConfiguration], "panda_ntt_slab_step2_bn254_enqueue": [NttSlabConfiguration],
        "panda_ntt_slab_inverse_step1_bn254_enqueue": [NttSlabConfiguration], "panda_ntt_slab_inverse_step2_bn254_enqueue": [NttSlabConfiguration],
        "panda_gen_scalars": [u, C.c_uint64, C.c_uint64, C.c_uint64, vp, PandaStream], "panda_gen_bases": [u, C.c_uint64, C.c_uint64, C.c_uint64, vp, PandaStream],
        "panda_debug_field_op": [u, u, vp, vp, vp, sz, PandaStream], "panda_debug_curve_op": [u, u, vp, vp, vp, sz, PandaStream],
        "panda_debug_fe_internal": [u, u, vp, vp, vp, vp, vp, sz, PandaStream],
        "panda_debug_xyzz_internal": [u, u, vp, vp, vp, sz, PandaStream],
        "panda_debug_scratch_fill": [u, u, C.POINTER(vp), C.POINTER(sz)],
        "panda_ntt_table_builds": [C.POINTER(C.c_uint64)], "panda_msm_set_chunk_first": [u], "panda_set_clock_stamps": [u], "panda_msm_last_clock": [C.POINTER(C.c_uint64)],
        "panda_ntt_last_clock": [C.POINTER(C.c_uint64)], "panda_clock_stamp": [PandaStream, vp], "panda_clock_delta": [vp, vp, C.POINTER(C.c_uint64)],
        "panda_multi_gpu_create": [C.POINTER(PandaMultiGpu), C.POINTER(C.c_int), u, u], "panda_multi_gpu_destroy": [PandaMultiGpu],
        "panda_multi_gpu_device_count": [PandaMultiGpu, C.POINTER(u)],
        "panda_msm_execute_bn254_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), vp], "panda_msm_execute_bls12_377_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), vp],
        "panda_msm_execute_bn254_from_host_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), C.POINTER(vp), u, vp],
        "panda_msm_execute_bls12_377_from_host_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), C.POINTER(vp), u, vp],
        "panda_msm_execute_bls12_381_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), vp], "panda_msm_execute_bn254_g2_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), vp],
        "panda_msm_execute_bls12_381_from_host_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), C.POINTER(vp), u, vp],
        "panda_msm_execute_bn254_g2_from_host_multi": [PandaMultiGpu, C.POINTER(MSMConfiguration), C.POINTER(vp), u, vp],
        "panda_ntt_execute_bn254_multi": [PandaMultiGpu, C.POINTER(NttSlabConfiguration)], "panda_ntt_execute_bn254_inverse_multi": [PandaMultiGpu, C.POINTER(NttSlabConfiguration)],
        "panda_ntt_execute_bn254_multi_batch": [PandaMultiGpu, C.POINTER(NttSlabConfiguration), C.c_uint], "panda_ntt_execute_bn254_inverse_multi_batch": [PandaMultiGpu, C.POINTER(NttSlabConfiguration), C.c_uint],
        "panda_multi_gpu_last_phase_ms": [PandaMultiGpu, u, C.POINTER(C.c_float)],
        "panda_ntt_execute_bls12_377_bitrev_out": [NttconfigurationV1], "panda_ntt_execute_bls12_377_inverse_bitrev_in": [NttconfigurationV1],
        "panda_ntt_execute_bls12_377_coset": [NttconfigurationV1, vp], "panda_ntt_execute_bls12_377_coset_inverse": [NttconfigurationV1, vp],
        "panda_ntt_slab_step1_bls12_377_enqueue": [NttSlabConfiguration], "panda_ntt_slab_step2_bls12_377_enqueue": [NttSlabConfiguration],
        "panda_ntt_slab_inverse_step1_bls12_377_enqueue": [NttSlabConfiguration], "panda_ntt_slab_inverse_step2_bls12_377_enqueue": [NttSlabConfiguration],
        "panda_ntt_execute_bls12_377_multi": [PandaMultiGpu, C.POINTER(NttSlabConfiguration)], "panda_ntt_execute_bls12_377_inverse_multi": [PandaMultiGpu, C.POINTER(NttSlabConfiguration)],
        "panda_ntt_execute_bls12_377_multi_batch": [PandaMultiGpu, C.POINTER(NttSlabConfiguration), C.c_uint],
        "panda_ntt_execute_bls12_377_inverse_multi_batch": [PandaMultiGpu, C.POINTER(NttSlabConfiguration), C.c_uint],
    }
    for name in [n for n in list(sig) if "bls12_377" in n and n.replace("bls12_377", "bls12_381") in ADDITIVE_SYMBOLS]:
        sig.setdefault(name.replace("bls12_377", "bls12_381"), sig[name])
    for name, args in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if LIB_PATH.endswith(os.path.join("csrc", "libpanda-cuda.so")):
                raise  # the in-tree build must export everything
            continue   # tools/*_bench.py pointed LIB_PATH at an earlier round's build (PANDA_LIB) for an A/B run
        fn.argtypes = args
        fn.restype = C.c_uint  # PandaError = c_uint, gpu_ffi/mod.rs:8
    lib.panda_msm_phase_name.argtypes = [u]
    lib.panda_msm_phase_name.restype = C.c_char_p
    lib.panda_version.argtypes = []
    lib.panda_version.restype = C.c_char_p
    _lib = lib
    return lib


def check(code: int, kind: str) -> None:
    if code != 0:
        raise PandaGpuError(kind, code)
