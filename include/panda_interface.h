/*
 * panda_interface.h -- the drop-in C ABI of the MI355X-native MSM + NTT library.
 *
 * Every declaration in part 1 replaces, symbol for symbol and struct layout for struct layout,
 * an `extern "C"` entry point of the reference's L2 shim so that the reference's Rust `gpu_ffi`
 * (src/gpu_ffi/binding.rs:3-115) binds to this library unchanged:
 *
 *   reference declaration            src/cuda/core/panda_interface.cuh:10-110
 *   reference definition             src/cuda/core/panda_interface.cu:11-191
 *   Rust-side extern block           src/gpu_ffi/binding.rs:3-115
 *   Rust-side repr(C) structs        src/gpu_ffi/common.rs:40-44,89-93,134-138,160-208
 *
 * Part 2 are the four symbols the Rust side declares but the reference never defines
 * (binding.rs:14,16,54-56).  Part 3 is additive (no reference counterpart): BLS12-377 / BLS12-381 / BN254 G2 / BLS12-381 G2 / BLS12-377 G2,
 * cached-base registration and tables, the in-call upload pipeline, inverse / coset / bit-reversed NTTs, batches, the low-degree
 * extension, polynomial evaluation and division by X - z, batch inversion and grand products over the scalar fields, fused sums of
 * products, logUp lookup support (multiplicities and running sums), sumcheck rounds over multilinear tables, sparse matrix-vector
 * products, the EC-NTT over G1 with batch affine normalisation of device points, multi-GPU halves and synthetic-input / diagnostics
 * entry points.
 *
 * Conventions (unchanged from the reference):
 *   - return value: the HIP runtime's error code cast to unsigned; 0 = success
 *     (panda_interface.cuh:10-16; Rust only tests `!= 0`, unit.rs:55,79)
 *   - handles are `{ void *handle; }` passed BY VALUE; handle = hipStream_t / hipEvent_t / hipMemPool_t
 *   - configuration structs are passed BY VALUE (48 / 48 / 56 bytes)
 *   - panda_msm_execute_* and panda_ntt_execute_* are synchronous on return
 *   - field elements: little-endian u32 limbs in Montgomery form; scalar 32 B; BN254 affine
 *     base 64 B (x||y, identity <=> x == 0); result 96 B X||Y||Z (Jacobian by default,
 *     homogeneous X/Z,Y/Z when PROJECTIVE is requested), identity <=> Z == 0
 *   - unlike the reference (msm_cuda.cuh:155, :554-555) the scalar buffer is never modified and
 *     the device is the caller's current device, not a hard-coded device 0.
 */
#ifndef PANDA_INTERFACE_H
#define PANDA_INTERFACE_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ part 1: reference ABI */

typedef enum panda_error /* panda_interface.cuh:10-16 */
{
    panda_success = 0,
    panda_error_invalid_value = 1,
    panda_error_memory_allocation = 2,
    panda_error_not_ready = 600
} panda_error;

typedef struct panda_stream { void *handle; } panda_stream;     /* panda_interface.cuh:18-21 */
typedef struct panda_event { void *handle; } panda_event;       /* panda_interface.cuh:23-26 */
typedef struct panda_mem_pool { void *handle; } panda_mem_pool; /* panda_interface.cuh:28-31 */

typedef enum panda_msm_result_coordinate_type /* panda_interface.cuh:33-37 */
{
    JACOBIAN = 0,
    PROJECTIVE,
} panda_msm_result_coordinate_type;

typedef void (*panda_host_fn)(void *user_data); /* panda_interface.cuh:39 */

/* runtime shim -- panda_interface.cuh:40-68, panda_interface.cu:11-154 */
panda_error panda_get_device_number(int *count);
panda_error panda_get_device(int *device_id);
panda_error panda_set_device(int device_id);
panda_error panda_stream_create(panda_stream *stream, bool blocking_sync);
panda_error panda_stream_wait_event(panda_stream stream, panda_event event);
panda_error panda_stream_sync(panda_stream stream);
panda_error panda_stream_destroy(panda_stream stream);
panda_error panda_launch_host_fn(panda_stream stream, panda_host_fn fn, void *user_data);
panda_error panda_event_create(panda_event *event, bool blocking_sync, bool disable_timing);
panda_error panda_event_record(panda_event event, panda_stream stream);
panda_error panda_event_sync(panda_event event);
panda_error panda_event_query(panda_event event);
panda_error panda_event_destroy(panda_event event);
panda_error panda_mem_get_info(size_t *free, size_t *total);
panda_error panda_malloc(void **ptr, size_t size);
panda_error panda_malloc_host(void **ptr, size_t size);
panda_error panda_free(void *ptr);
panda_error panda_free_host(void *ptr);
panda_error panda_host_register(void *ptr, size_t size);
panda_error panda_host_unregister(void *ptr);
panda_error panda_memcpy(void *dst, const void *src, size_t count);
panda_error panda_memcpy_async(void *dst, const void *src, size_t count, panda_stream stream);
panda_error panda_memset(void *ptr, int value, size_t count);
panda_error panda_memset_async(void *ptr, int value, size_t count, panda_stream stream);
panda_error panda_mem_pool_create(panda_mem_pool *pool, int device_id);
panda_error panda_mem_pool_destroy(panda_mem_pool pool);
panda_error panda_malloc_from_pool_async(void **ptr, size_t size, panda_mem_pool pool, panda_stream stream);
panda_error panda_free_async(void *ptr, panda_stream stream);

typedef struct panda_msm_configuration /* panda_interface.cuh:70-79; Rust MSMConfiguration common.rs:168-185 */
{
    panda_mem_pool mem_pool;
    panda_stream stream;
    void *bases;   /* device: n affine points */
    void *scalars; /* device: n Montgomery-form Fr; read-only here */
    void *results; /* device or pinned host: 3 field elements */
    unsigned log_scalars_count;
    panda_msm_result_coordinate_type msm_result_coordinate_type;
} panda_msm_configuration;
typedef panda_msm_configuration msm_configuration;

panda_error panda_msm_setup_bn254(void);                                               /* panda_interface.cu:152-155 */
panda_error panda_msm_execute_bn254(const panda_msm_configuration exec_cfg);           /* panda_interface.cu:157-160 -> msm_cuda.cuh:551-784 */
panda_error panda_msm_execute_bn254_host(const panda_msm_configuration exec_cfg);      /* panda_interface.cu:162-165 -> msm_host.cuh:267-383; all pointers host */
panda_error panda_msm_tear_down(void);                                                 /* panda_interface.cu:167-170 */

typedef struct panda_ntt_configuration /* panda_interface.cuh:86-94; Rust NTTConfiguration common.rs:187-196 */
{
    panda_mem_pool mem_pool;
    panda_stream stream;
    void *d_src;
    void *d_dst;
    unsigned log_n;
    void *flag; /* host unsigned*: 0 -> result in d_src, 1 -> result in d_dst (fft.cu:211, unit.rs:521-532) */
} panda_ntt_configuration;
typedef panda_ntt_configuration ntt_configuration;

typedef struct panda_ntt_configuration_v1 /* panda_interface.cuh:96-105; Rust NttconfigurationV1 common.rs:198-208 */
{
    panda_mem_pool mem_pool;
    panda_stream stream;
    void *d_src;
    void *d_dst;
    void *d_omega; /* HOST pointer to one Montgomery-form Fr: the primitive 2^log_n-th root (unit.rs:501-511) */
    unsigned log_n;
    void *flag;
} panda_ntt_configuration_v1;
typedef panda_ntt_configuration_v1 ntt_configuration_v1;

panda_error panda_ntt_setup_bn254(void *input_omega);                                  /* panda_interface.cu:172-176 -> fft.cu:225-229 */
panda_error panda_ntt_execute_bn254(panda_ntt_configuration exec_cfg);                 /* panda_interface.cu:178-181 -> fft.cu:231-242 */
panda_error panda_ntt_tear_down(void);                                                 /* panda_interface.cu:188-191 */
panda_error panda_ntt_execute_bn254_v1(const panda_ntt_configuration_v1 exec_cfg);     /* panda_interface.cu:183-186 -> fft.cu:244-260 */

/* ------------------------------------------- part 2: declared by Rust, undefined in the reference */

panda_error panda_stream_synchronize(panda_stream stream); /* binding.rs:14; used by PandaStream::sync, common.rs:71-76 */
panda_error panda_stream_query(panda_stream stream);       /* binding.rs:16 (also declared in panda_interface.cuh:46) */
panda_error panda_device_enable_peer_access(int device_id);  /* binding.rs:56 */
panda_error panda_device_disable_peer_access(int device_id); /* binding.rs:54 */

/* ------------------------------------------------------------------ part 3: additive entry points */

/* BLS12-377 G1 MSM: bases 96 B affine, scalars 32 B, result 144 B (README.md:36 roadmap; BASELINE config 5) */
panda_error panda_msm_setup_bls12_377(void);
panda_error panda_msm_execute_bls12_377(const panda_msm_configuration exec_cfg);
panda_error panda_msm_execute_bls12_377_host(const panda_msm_configuration exec_cfg);
/* BLS12-381 G1 (the reference names the curve, curve.cuh:12, but carries no parameters for it): bases 96 B, result 144 B, curve id 2 */
panda_error panda_msm_setup_bls12_381(void);
panda_error panda_msm_execute_bls12_381(const panda_msm_configuration exec_cfg);
panda_error panda_msm_execute_bls12_381_host(const panda_msm_configuration exec_cfg);

/* BN254 G2 (no counterpart in the reference): the twist y^2 = x^3 + 3/(9+u) over Fq2 = Fq[u]/(u^2+1), scalars as for G1.
 * An Fq2 element is c0 || c1 (2 x 32 B, Montgomery form); affine base x || y = 128 B (identity <=> x == 0), result X || Y || Z = 192 B.
 * Curve id 3 wherever a curve id is taken (register / precompute / execute_from_host / gen_bases / debug_curve_op). */
panda_error panda_msm_setup_bn254_g2(void);
panda_error panda_msm_execute_bn254_g2(const panda_msm_configuration exec_cfg);
panda_error panda_msm_execute_bn254_g2_host(const panda_msm_configuration exec_cfg);
panda_error panda_msm_combine_bn254_g2(const void *partials, unsigned count, panda_msm_result_coordinate_type out_type, void *result);

/* BLS12-381 G2 (no counterpart in the reference): the twist y^2 = x^3 + 4(1 + u) over Fq2 = Fq[u]/(u^2+1), scalars of BLS12-381 Fr as
 * for G1.  An Fq2 element is c0 || c1 (2 x 48 B, Montgomery form); affine base x || y = 192 B (identity <=> x == 0), result X || Y || Z =
 * 288 B.  Curve id 4 wherever a curve id is taken (register / precompute / execute_from_host / gen_bases / gen_scalars / debug_curve_op).
 * Bases are not checked for membership in the order-r subgroup (as for BN254 G2): that is the caller's business.  The accumulation
 * kernel ships in one shape for this curve: panda_msm_set_accumulate_variant and panda_msm_set_overlap have no effect on it. */
panda_error panda_msm_setup_bls12_381_g2(void);
panda_error panda_msm_execute_bls12_381_g2(const panda_msm_configuration exec_cfg);
panda_error panda_msm_execute_bls12_381_g2_host(const panda_msm_configuration exec_cfg);
panda_error panda_msm_combine_bls12_381_g2(const void *partials, unsigned count, panda_msm_result_coordinate_type out_type, void *result);

/* BLS12-377 G2 (no counterpart in the reference): the twist y^2 = x^3 + 1/u over Fq2 = Fq[u]/(u^2+5) (-1 is a square mod this p), scalars
 * of BLS12-377 Fr as for G1.  Wire format as for BLS12-381 G2: an Fq2 element is c0 || c1 (2 x 48 B, Montgomery form); affine base
 * x || y = 192 B (identity <=> x == 0), result X || Y || Z = 288 B.  Curve id 6 wherever a curve id is taken (id 5 is unused and refused).
 * Bases are not checked for membership in the order-r subgroup.  One shape of the accumulation kernel, as for BLS12-381 G2. */
panda_error panda_msm_setup_bls12_377_g2(void);
panda_error panda_msm_execute_bls12_377_g2(const panda_msm_configuration exec_cfg);
panda_error panda_msm_execute_bls12_377_g2_host(const panda_msm_configuration exec_cfg);
panda_error panda_msm_combine_bls12_377_g2(const void *partials, unsigned count, panda_msm_result_coordinate_type out_type, void *result);

/* Cached bases (README.md "Supports cached bases and scalars"; init_msm, wrapper.rs:122-152): registering a device buffer
 * of 2^log_n affine bases lets the library keep its radix-converted copy between calls instead of re-deriving it in every
 * panda_msm_execute_*; the caller must not modify the buffer until panda_msm_unregister_bases.  curve: 0 BN254, 1 BLS12-377, 2 BLS12-381, 3 BN254 G2,
 * 4 BLS12-381 G2, 6 BLS12-377 G2. */
panda_error panda_msm_register_bases(unsigned curve, const void *d_bases, unsigned log_n, panda_stream stream);
panda_error panda_msm_unregister_bases(const void *d_bases);
/* Strict staleness check of a registration: recomputes the 64-bit hash of the whole wire buffer (one streaming pass, about 0.2 ms
 * per GiB; synchronises `stream`) and compares it with the hash taken when the buffer was registered.  panda_success: unchanged;
 * panda_error_invalid_value: not registered, or changed -- the registration has then been dropped.  (Every execute additionally
 * compares 64 sampled rows at no cost; that catches wholesale reuse of the address, not a change confined to other rows.) */
panda_error panda_msm_verify_registered(const void *d_bases, panda_stream stream);
/* on != 0: every panda_msm_execute_* against registered bases runs panda_msm_verify_registered's check first */
panda_error panda_msm_set_paranoid(unsigned on);
/* Cached bases with precomputed window tables (the lookup-table idea the reference left as a stub, msm_host.cuh:248-265):
 * besides the converted copy the library keeps 2^lo[k] * P for every window k (W tables of 2^log_n affine rows, built once,
 * about W * 64 B per BN254 point).  Every window then shares one bucket space, which permits windows of up to 23 bits and
 * removes the per-window reductions.  window_bits 0 = built-in policy.  Results are the same group element as without tables.
 * Undone by panda_msm_unregister_bases. */
panda_error panda_msm_precompute_bases(unsigned curve, const void *d_bases, unsigned log_n, unsigned window_bits, panda_stream stream);
/* what is registered for d_bases: number of tables (1 = converted copy only), window bits (0 if none), device bytes held */
panda_error panda_msm_registered_info(const void *d_bases, unsigned *tables, unsigned *window_bits, size_t *bytes);

/* Upload / execute pipeline inside ONE call (the reference's h2d / exec streams, wrapper.rs:260-273 and unit.rs:17-29, run
 * one after the other).  exec_cfg is as for panda_msm_execute_*; exec_cfg.scalars is the caller's DEVICE buffer of n x 32 bytes and
 * h_scalars the HOST source it is filled from (pinned memory lets the copies run beside the kernels).  Against registered bases the
 * scalars are cut into `ranges` (1..8) contiguous point ranges of n/2^(R-1), n/2^(R-1), n/2^(R-2), ..., n/2 points: range r+1 is copied
 * on h2d_stream while range r runs digits -> sort -> accumulate on exec_cfg.stream against its own rows of the registered tables; each
 * range's buckets are added into a running total on the device, which is reduced once.  Unregistered bases, or fewer than 2^16 points
 * in the first range, reduce the number of ranges, down to one copy followed by the ordinary call.  h_scalars == NULL skips the copies
 * and runs the same schedule on resident scalars.  Synchronous on return like panda_msm_execute_*; same group element.  curve: 0 .. 4, 6
 * (BN254, BLS12-377, BLS12-381, BN254 G2, BLS12-381 G2, BLS12-377 G2).  Experiment switch: ranges = 0x100 | R with h_scalars == NULL runs R (a power of two) EQUAL ranges
 * one after the other on the caller's stream (the table-footprint measurement of profiles/r05_accumulate_table_footprint.txt). */
panda_error panda_msm_execute_from_host(unsigned curve, const panda_msm_configuration exec_cfg, const void *h_scalars, unsigned ranges, panda_stream h2d_stream);

/* `batch` MSMs over ONE base set in one call: the shape a prover calls an MSM in (every commitment of a round goes against the same SRS).
 * exec_cfg is as for panda_msm_execute_*: bases = 2^log_scalars_count affine points; scalars = batch x 2^log_scalars_count x 32 B on the
 * device, member j at byte offset j * 2^log_scalars_count * 32, read-only; results = batch x (96 / 144 / 192 / 288) B, member j at
 * j * result bytes, device or pinned host or pageable host; msm_result_coordinate_type applies to every member.  Synchronous on return.
 * Member j's result is the same group element as panda_msm_execute_* on member j alone; the raw bytes are ONE representative of it
 * (Jacobian / homogeneous coordinates are defined up to a factor, and the order in which a bucket's points are added follows the wave
 * scheduling -- true of the single call as well): compare affine points, never bytes.  curve: 0 .. 4, 6.
 *   batch: 1 .. PANDA_MSM_MAX_BATCH.  batch == 0 or above the maximum, curve 5 or > 6, log_scalars_count > 26, NULL buffers, and scalar /
 *     result buffers of this library's allocators that are shorter than `batch` members return panda_error_invalid_value, nothing
 *     launched; the batch == 0 / curve / NULL checks come before any runtime call.
 *   Bases with precomputed tables (panda_msm_precompute_bases): the FUSED path.  The batch is cut into groups of a power-of-two number of
 *     members (13 = 8 + 4 + 1; the largest group is what panda_msm_batch_plan reports), and a group runs as one MSM of group x n scalars
 *     whose bucket id carries the member index: one digits pass, one sort, one accumulation and one fix-up for the group, one reduction
 *     that emits the group's results.  The tables' window plan is used as registered.
 *   Registered without tables, or not registered: the members run one after the other through the path of the single call.
 *   A registration found stale (sampled rows, or the hash under panda_msm_set_paranoid) is dropped and the WHOLE batch answered from the
 *     caller's buffer, as a single call does.
 *   The experiment setters (panda_msm_set_overlap, _accumulate_variant, _wide_merge, _chunk_first, point ranges) have no effect on the fused
 *     path, which ships in the built-in shape of each curve; panda_msm_set_window_bits and _chunk_entries keep their meaning for the
 *     unfused path only.  panda_msm_last_phase_ms after a fused batch reports the LAST group: its device time in "total_device" (under
 *     panda_msm_set_phase_timing(1) or (2)), the other phases 0; after an unfused batch, the last member. */
#define PANDA_MSM_MAX_BATCH 1024
panda_error panda_msm_execute_batch(unsigned curve, const panda_msm_configuration exec_cfg, unsigned batch);
/* How a batch would run (pure host arithmetic, no device call): window_bits = the window of the precomputed tables
 * (panda_msm_registered_info), 0 = the built-in tabled policy for 2^log_n points.  *group_log = log2 of the largest number of members
 * fused into one sort + accumulate (0: members run one after the other), *sequences = number of kernel sequences the whole batch is cut
 * into.  Either pointer may be NULL.  Invalid: curve 5 or > 6, log_n > 26, batch 0 or > PANDA_MSM_MAX_BATCH, window_bits 1 .. 3 or > 24. */
panda_error panda_msm_batch_plan(unsigned curve, unsigned log_n, unsigned window_bits, unsigned batch, unsigned *group_log, unsigned *sequences);

/* Window size override for experiments: 0 = built-in policy (replaces get_window_bits_count, msm_cuda.cuh:21-45) */
panda_error panda_msm_set_window_bits(unsigned window_bits);
/* what the plain path (no precomputed tables) would run a 2^log_n-point MSM of `curve` with: widest window and number of windows */
panda_error panda_msm_plain_window_plan(unsigned curve, unsigned log_n, unsigned *window_bits, unsigned *windows);
/* sorted entries per thread of the bucket-accumulation kernel, for experiments: 0 = built-in policy (rounded up to a multiple of 4) */
panda_error panda_msm_set_chunk_entries(unsigned entries);
/* With precomputed tables, levels 2 and 3 of the bucket sort for all but the first front_of_128 / 128 of the bucket space run on a second
 * stream of the calling host thread, beside the accumulation of that front part; the rest is then accumulated on that second stream.
 * workgroups_per_cu = 64: the front's accumulation is an ordinary grid; less: that many workgroups per CU whose waves draw their chunks
 * from a counter; 0 = built-in (8 for BN254).  front_of_128: 1 .. 127, 0 = one stream, one phase after the other, 0xffffffff = built-in
 * policy (default: off -- every schedule measured is slower on MI355X, profiles/r05_overlap_sort_accumulate.txt).  Same group element. */
panda_error panda_msm_set_overlap(unsigned front_of_128, unsigned workgroups_per_cu);
/* Experiments on the bucket-accumulation kernel of the 9-limb base fields (BN254): 0 = the built-in choice, 1 = five waves per SIMD with
 * the next entry's table row staged in LDS (global_load_lds) instead of registers, 2 = four waves per SIMD with the staged row, 3 = (every
 * curve) the rows of a wave fetched four lanes to a row into LDS (profiles/r05_accumulate_table_footprint.txt), 4 = (every curve) a
 * chunk's sorted words in whole 64-byte sectors through LDS -- built in for the 9-limb fields from round 6 on --, 5 = never (sixteen-byte
 * global loads, as rounds 2-5 did; profiles/r06_accumulate_fetch_and_row_loads.txt).  Same group element. */
panda_error panda_msm_set_accumulate_variant(unsigned variant);
/* Level-3 merge of the bucket sort (tabled calls): 0 = built-in (the cells of the lower half of the bucket space, which hold up to twice
 * the mean when the plan mixes two window widths, go through the variant that reads up to 32 k entries per cell once, those of the upper
 * half through 256-thread workgroups), 1 = every cell through the wide variant, 2 = neither variant, 3 = every cell through the 256-thread
 * variant (profiles/r05_k3_merge_cells.txt).  Same group element. */
panda_error panda_msm_set_wide_merge(unsigned mode);
/* deprecated no-op kept so that code linked against the round-3 interface still loads (the bucket reduction has no groups any more) */
panda_error panda_msm_set_reduce_group(unsigned log_group);
/* 1 (built in): a small kernel behind the sort hands every chunk of the bucket-accumulation kernel the bucket its first entry falls in;
 * 0: every thread of that kernel finds it by binary search over the bucket offsets, as rounds 1-5 did (A/B measurements). */
panda_error panda_msm_set_chunk_first(unsigned on);
/* Which device timers a call records (an event between two kernels keeps the GPU idle for about 6 us): 0 = none (default),
 * 1 = the call's total + the bucket-accumulation kernel, 2 = every phase.  Phases that were not timed read 0 in panda_msm_last_phase_ms. */
panda_error panda_msm_set_phase_timing(unsigned level);
/* per-phase device times of the last MSM on this thread, milliseconds; names via panda_msm_phase_name */
#define PANDA_MSM_PHASES 8
panda_error panda_msm_last_phase_ms(float *ms /* PANDA_MSM_PHASES floats */);
const char *panda_msm_phase_name(unsigned phase);

/* Inverse transform: runs the forward passes with omega^-1 and fuses the n^-1 scaling into the last pass.
 * d_omega is the FORWARD root (host pointer), as for _v1. */
panda_error panda_ntt_execute_bn254_inverse(const panda_ntt_configuration_v1 exec_cfg);
/* device time of the passes of the last panda_ntt_execute_* on this host thread (HIP events on the launch stream), milliseconds */
panda_error panda_ntt_last_device_ms(float *ms);
/* The passes a natural-order transform of 2^log_n points runs: their number (the reference's loop, fft.cu:171-216, takes eight bits per
 * pass; here 2^17/2^18 and 2^25..2^27 run one pass less behind radix-512 passes) and, if radix_bits != NULL, the bits of each (four
 * entries, zero-padded).  *flag of the execute calls is passes & 1.  The bit-reversed orderings run the same number of passes (radix-512
 * passes last for a bit-reversed input) except at 2^18 and 2^27, where they keep the eight-bit plan. */
panda_error panda_ntt_pass_plan(unsigned log_n, unsigned *passes, unsigned *radix_bits);
/* Streamed inter-pass table: the second boundary of a three-pass transform (2^17 .. 2^26 points) multiplies every element by ONE entry of
 * a table over the whole twiddle index range -- 32 bytes per element of the transform, built once per root, size and direction, kept in
 * the calling thread's twiddle cache (two slots) until panda_ntt_tear_down -- instead of by two entries of 2^16-entry tables.
 *   mode 1 (the default policy): transforms of 2^17 .. 2^24 points; the table is as large as the data, at most 512 MiB per slot, so one host
 *          thread that alternates forward and inverse 2^24-point transforms holds 1 GiB of tables (-6 % at 2^20, -4 % at 2^22, -1.4 % at 2^24)
 *   mode 2: also 2^25 / 2^26 points (1 GiB / 2 GiB per slot, up to 4 GiB per thread; -1.7 % / -0.9 %) -- opt-in
 *   mode 0: off (two small tables, as before round 5);  0xffffffff: back to the built-in policy;  3: test hook (allocation treated as failed)
 * A table that does not fit in free HBM is skipped for that size and device from then on (per host thread); the call still succeeds. */
panda_error panda_ntt_set_streamed_tables(unsigned mode);
/* whole-transform twiddle-table sets built so far by the calling host thread: a repeated transform must not add to it (cache hit) */
panda_error panda_ntt_table_builds(uint64_t *count);
/* `batch` transforms of 2^log_n points over one field with one root in ONE call: every pass is launched once over all members, with one
 * table set and one synchronisation -- the shape a prover's round transforms its polynomials in.
 *   field: 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr.  kind: which single call a member runs as (below).
 *   exec_cfg is the single call's struct.  d_src and d_dst are device buffers of batch x 2^log_n x 32 bytes, member j at byte offset
 *     j x 2^log_n x 32 of either; d_omega is the HOST pointer to the FORWARD root for every kind; `shift` the HOST pointer to the coset
 *     generator (32 bytes, Montgomery form, non-zero) for the coset kinds, ignored otherwise (may be NULL).
 *   *flag is what the single call of that kind and size writes (passes & 1 of the plan that kind runs): all members' results are in d_src
 *     (0) or in d_dst (1), member after member; the other buffer is scratch.  Member j's output is byte for byte what the single call of
 *     that kind writes for member j alone.  Synchronous on return.  Bytes outside the `batch` members are never written.
 *   Members of fewer than 2^10 points share a workgroup (1024 >> log_n whole members each, fewer in the last one); from 2^11 points on
 *     the grid of every pass kernel covers batch x tiles-per-member tiles.  The coset kinds apply the shift as one sweep over the whole
 *     batch in front of (forward) or behind (inverse) the passes.  log_n == 0 transforms nothing (flag 0).
 *   The twiddle tables are the calling thread's whole-transform cache under the single call's key: a batch after a single call of the
 *     same field, size, kind and root builds nothing, and the other way round; the streamed-table policy applies per member size (one
 *     table as large as ONE member serves all).  panda_ntt_last_device_ms / panda_ntt_last_clock report the batch's passes.
 *   panda_error_invalid_value, nothing launched: field > 2, kind > 5, batch == 0 or > PANDA_NTT_MAX_BATCH, log_n > 28, batch x 2^log_n >
 *     2^28 elements, NULL d_src / d_dst / d_omega / flag, NULL or zero shift for a coset kind (all checked before any runtime call), and
 *     d_src / d_dst of this library's allocators shorter than `batch` members. */
#define PANDA_NTT_MAX_BATCH 4096
#define PANDA_NTT_FORWARD 0u            /* panda_ntt_execute_<field>_v1 */
#define PANDA_NTT_INVERSE 1u            /* ..._inverse (n^-1 fused) */
#define PANDA_NTT_BITREV_OUT 2u         /* ..._bitrev_out */
#define PANDA_NTT_INVERSE_BITREV_IN 3u  /* ..._inverse_bitrev_in */
#define PANDA_NTT_COSET 4u              /* ..._coset */
#define PANDA_NTT_COSET_INVERSE 5u      /* ..._coset_inverse */
panda_error panda_ntt_execute_batch(unsigned field, unsigned kind, const panda_ntt_configuration_v1 exec_cfg, unsigned batch, const void *shift);
/* How a batch runs (pure host arithmetic, no device call): *launches = the transform kernels one call enqueues once its tables are
 * cached -- the passes of that kind and size (panda_ntt_pass_plan; the bit-reversed kinds keep the eight-bit plan at 2^18 / 2^27), plus
 * one for a coset kind's sweep -- whatever `batch` is; *members_per_workgroup = the members one workgroup of the first pass carries (1 from
 * 2^10 points on).  Either pointer may be NULL.  Invalid for the shapes panda_ntt_execute_batch refuses. */
panda_error panda_ntt_batch_plan(unsigned log_n, unsigned kind, unsigned batch, unsigned *launches, unsigned *members_per_workgroup);
/* Low-degree extension: `batch` polynomials of n = 2^log_n coefficients each to their evaluations on the coset g H_N of the domain of
 * N = B n points, B = 2^log_blowup -- what a prover does to every wire, selector and permutation polynomial before it forms the quotient.
 * f(g w_N^(i + B k)), k < n, is the n-point transform with root w_N^B of c_j (g w_N^i)^j, so the call runs B n-point members per
 * polynomial (the batch's passes, one launch per pass over all of them) instead of one N-point transform of mostly zeros: log_blowup
 * butterfly layers fewer, and no memset, copy or sweep over the zero padding.
 *   field: 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr.  exec_cfg.log_n is the log of the COEFFICIENT count.
 *   d_coeffs: device buffer of batch x n x 32 bytes, polynomial p at byte offset p x n x 32; read only.  exec_cfg.d_src and d_dst: device
 *     buffers of batch x N x 32 bytes each, neither overlapping d_coeffs.  exec_cfg.d_omega: HOST pointer to the primitive N-th root w_N
 *     of the EXTENDED domain (the members' root w_N^B is derived inside); `shift`: HOST pointer to g (32 bytes, Montgomery form, non-zero).
 *   order PANDA_NTT_LDE_COSET_MAJOR: element (p B + i) n + k is f_p(g w_N^(i + B k)), i < B, k < n -- the B cosets of the small domain one
 *     after the other; on coset i the vanishing polynomial X^n - 1 is the constant g^n w_N^(i n) - 1.
 *   order PANDA_NTT_LDE_NATURAL: element p N + m is f_p(g w_N^m): byte for byte what panda_ntt_execute_<field>_coset writes for c_p
 *     zero-padded to N points with root w_N and shift g (one more streaming kernel); the layout panda_ntt_execute_<field>_coset_inverse
 *     at size N takes a quotient back to coefficients from.
 *   *flag: 0 = the results are in d_src, 1 = in d_dst (panda_ntt_lde_plan tells in advance); the other buffer is scratch.  Outputs are
 *     canonical.  Bytes behind the `batch` polynomials of any of the three buffers are never written.  Synchronous on return.
 *   The members' twiddle tables are the calling thread's whole-transform cache under the single call's key for (log_n, forward, w_N^B): a
 *     panda_ntt_execute_<field>_v1 call of 2^log_n points with that root after an extension builds nothing, and the other way round.  The
 *     power tables of g are the ones a forward coset batch of 2^log_n points with that shift caches; those of w_N are cached by field,
 *     log_n, log_blowup and root.  panda_ntt_last_device_ms / panda_ntt_last_clock report the passes.  log_n == 0 is legal.
 *   panda_error_invalid_value, nothing launched, *flag untouched: field > 2, order > 1, log_blowup == 0 or > PANDA_NTT_LDE_MAX_LOG_BLOWUP,
 *     batch == 0, batch x B > PANDA_NTT_MAX_BATCH, batch x N > 2^28 elements, log_n > 28, NULL d_coeffs / d_src / d_dst / d_omega / flag,
 *     NULL or zero shift, d_coeffs overlapping d_src or d_dst as address ranges (all checked before any runtime call), and buffers of this
 *     library's allocators shorter than stated. */
#define PANDA_NTT_LDE_MAX_LOG_BLOWUP 4
#define PANDA_NTT_LDE_COSET_MAJOR 0u
#define PANDA_NTT_LDE_NATURAL 1u
panda_error panda_ntt_execute_lde(unsigned field, const panda_ntt_configuration_v1 exec_cfg, const void *d_coeffs, unsigned log_blowup, unsigned batch,
                                  const void *shift, unsigned order);
/* How an extension runs (pure host arithmetic): *launches = 1 (expand) + the passes of 2^log_n points (panda_ntt_pass_plan) + 1 for the
 * NATURAL order's interleave; *flag = the value panda_ntt_execute_lde will write, (passes + order) & 1.  Neither depends on `batch`.
 * Either pointer may be NULL.  Invalid for the shapes panda_ntt_execute_lde refuses. */
panda_error panda_ntt_lde_plan(unsigned log_n, unsigned log_blowup, unsigned batch, unsigned order, unsigned *launches, unsigned *flag);
/* KZG openings: evaluation of `batch` polynomials at a few points, and their division by X - z -- what a prover does with the coefficients
 * an inverse transform left on the device, between that transform and the MSM that commits to the opening quotient.  With the suffix
 * Horner values S_j = sum_{i >= j} c_i z^(i-j) (S_j = c_j + z S_(j+1), S_n = 0): f(z) = S_0, and (f(X) - f(z)) / (X - z) has the
 * coefficients q_j = S_(j+1), j < n - 1; q_(n-1) = 0 is written as well, so the quotient has n elements and is ready for an MSM of the
 * same size (panda_msm_execute_* take it as their scalars as it stands).
 *   field: 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr.  Elements are 32-byte little-endian Montgomery-form residues; polynomial p starts at
 *     byte p x n x 32 of d_coeffs and of d_quot.  n is ANY count from 1 up, not a power of two (blinded polynomials have 2^k + 2 or 2^k + 3
 *     coefficients).  batch >= 1, batch x n <= 2^28.
 *   points / point: HOST pointers (n_points x 32 B / 32 B), like d_omega and shift; a point's 256-bit value must be below the modulus.
 *   values (HOST, batch x n_points x 32 B): f_p(z_k) at element p x n_points + k.  remainders (HOST, batch x 32 B, may be NULL): f_p(z).
 *   Outputs are canonical.  Both calls are synchronous on return and read d_coeffs only; d_quot == d_coeffs exactly (division in place) is
 *     legal.  Bytes behind the `batch` polynomials of either buffer are never written.
 *   Division is three kernel launches (tile totals; one workgroup per polynomial over the totals; apply), evaluation the first two, once
 *     per point; no kernel waits for another workgroup.  The scratch (32 bytes per tile and per value) is the calling host thread's arena: a
 *     repeated call of the same shape allocates nothing, panda_ntt_tear_down releases it.
 *   panda_error_invalid_value, nothing launched, no output written: field > 2, n == 0, batch == 0, batch x n > 2^28, n_points == 0 or >
 *     PANDA_POLY_MAX_POINTS, a NULL buffer or point other than remainders, a point >= the modulus, d_quot and d_coeffs overlapping as
 *     address ranges without being equal (all checked before any runtime call), and buffers of this library's allocators shorter than
 *     stated. */
#define PANDA_POLY_MAX_POINTS 8
panda_error panda_poly_evaluate(unsigned field, const void *d_coeffs, uint64_t n, unsigned batch, const void *points /* HOST, n_points x 32 B */, unsigned n_points,
                                void *values /* HOST, batch x n_points x 32 B */, panda_stream stream);
panda_error panda_poly_divide_linear(unsigned field, const void *d_coeffs, void *d_quot, uint64_t n, unsigned batch, const void *point /* HOST, 32 B */,
                                     void *remainders /* HOST, batch x 32 B, may be NULL */, panda_stream stream);
/* How the two calls run (pure host arithmetic, no device call): *tile = the coefficients one workgroup covers, *carry_chunk = the tile
 * totals the second level combines per step, *launches_evaluate = the kernel launches of one sweep over the coefficients (one sweep per
 * point), *launches_divide = those of a division.  None depends on `batch`.  Any pointer may be NULL.  Invalid for the shapes the execute
 * calls refuse (n == 0, batch == 0, batch x n > 2^28). */
panda_error panda_poly_plan(uint64_t n, unsigned batch, unsigned *tile, unsigned *carry_chunk, unsigned *launches_evaluate, unsigned *launches_divide);
/* KZG openings of polynomials held as EVALUATIONS (EIP-4844 blobs, PeerDAS cells, Plonk with a Lagrange SRS): the same two steps as the pair
 * above without a transform.  n = 2^log_n, w = omega a primitive n-th root, s = shift (NULL: 1) the coset shift, x_i = s w^i.  Position j of
 * a vector holds e_j = f(x_sigma(j)), sigma the identity (PANDA_DOMAIN_NATURAL) or the bit reversal over log_n bits (PANDA_DOMAIN_BITREV);
 * f is the polynomial of degree < n with those values.
 *   value:     z^n != s^n: with u = z / s, f(z) = (u^n - 1) / n  sum_i e_i w^i / (u - w^i).  z^n == s^n: z = x_m for one m and f(z) = e_m,
 *              copied, not computed -- exact at domain points (a challenge may be a root of unity).
 *   quotient:  q(X) = (f(X) - f(z)) / (X - z), of degree < n - 1, in the form, domain and order of the input: q_i = (e_i - f(z)) / (x_i - z)
 *              for x_i != z and q_m = -(1 / z) sum_{i != m} q_i x_i at x_m = z.  It is what the MSM takes as scalars: against the Lagrange
 *              SRS of the same domain and order (panda_ec_ntt, inverse) that MSM is the opening proof.
 *   field: 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr.  Elements are 32-byte little-endian Montgomery-form residues; vector p starts at byte
 *     p x n x 32 of d_evals and of d_quot.  batch >= 1, batch x n <= 2^28; log_n == 0 is legal (the value is e_0, the quotient 0).
 *   omega, shift, points / point: HOST pointers (32 B each, points n_points x 32 B), values below the modulus.  Points of one call may lie on
 *     and off the domain and may repeat.  values (HOST, batch x n_points x 32 B): f_p(z_k) at element p x n_points + k.  remainders (HOST,
 *     batch x 32 B, may be NULL): f_p(z).
 *   Outputs are canonical and the same bytes on every run.  Both calls are synchronous on return; d_quot == d_evals exactly (division in
 *     place) is legal, otherwise d_evals is only read.  Bytes behind the `batch` vectors of either buffer are never written.
 *   The domain points and the denominators are computed in the kernels; the host decides z^n == s^n and finds m (log_n steps in the
 *     2-group).  The denominators are inverted by the product trick with ONE field inversion per call, on the host, for n and all points
 *     together (the grand product of a point's denominators is u^n - 1, or n / u at a domain point); a call with a shift inverts the
 *     shift as well.  Evaluation is four kernel launches for all points together and reads d_evals once; division is five.  Every
 *     further point of an evaluation repeats the inverses: for several points of one polynomial the coefficient-form pair is cheaper.
 *     No kernel waits for another workgroup.  The scratch (32 bytes per tile, vector and point, and per value) is the calling host
 *     thread's arena: a repeated call of the same shape allocates nothing, panda_ntt_tear_down releases it.  It never exceeds 64 MiB + 64
 *     bytes per tile and point: a batch whose vectors x tiles x points exceed 2^21 (only vectors of fewer than 2^11 elements can) runs
 *     in slices of that many, each with the launches behind the first two of its own.
 *   panda_error_invalid_value, nothing launched, no output written: field > 2, log_n > 28, batch == 0, batch x n > 2^28, order > 1, n_points
 *     == 0 or > PANDA_POLY_MAX_POINTS, a NULL buffer, root or point (shift and remainders may be NULL), omega, shift or a point >= the
 *     modulus, shift == 0, omega not primitive (omega^(n/2) != -1; omega != 1 for log_n == 0), d_quot and d_evals overlapping as address
 *     ranges without being equal (all checked before any runtime call), and buffers of this library's allocators shorter than stated. */
#define PANDA_DOMAIN_NATURAL 0u
#define PANDA_DOMAIN_BITREV 1u
panda_error panda_poly_evaluate_lagrange(unsigned field, const void *d_evals, unsigned log_n, unsigned batch, const void *omega /* HOST, 32 B */,
                                         const void *shift /* HOST, 32 B, may be NULL */, unsigned order, const void *points /* HOST, n_points x 32 B */,
                                         unsigned n_points, void *values /* HOST, batch x n_points x 32 B */, panda_stream stream);
panda_error panda_poly_divide_linear_lagrange(unsigned field, const void *d_evals, void *d_quot, unsigned log_n, unsigned batch, const void *omega /* HOST, 32 B */,
                                              const void *shift /* HOST, 32 B, may be NULL */, unsigned order, const void *point /* HOST, 32 B */,
                                              void *remainders /* HOST, batch x 32 B, may be NULL */, panda_stream stream);
/* How the two calls run (pure host arithmetic, no device call): *tile = the positions one workgroup covers; the kernels that run one
 * workgroup per point or vector combine *tile / 2 per-tile partials per step, so they take a second step from tile x tile / 2 positions
 * on (2^22 for a tile of 2^11).  *launches_evaluate and *launches_divide = the kernel launches of a call (of a call's only slice, see
 * above), *inversions_per_vector_and_point = an upper bound on the field inversions behind one value or quotient: there is one per
 * call, on the host, and one more for a shift.  None depends on `batch`.  Any pointer may be NULL.  Invalid for the shapes the execute
 * calls refuse (log_n > 28, batch == 0, batch x n > 2^28, n_points == 0 or > PANDA_POLY_MAX_POINTS). */
panda_error panda_poly_lagrange_plan(unsigned log_n, unsigned batch, unsigned n_points, unsigned *tile, unsigned *launches_evaluate, unsigned *launches_divide,
                                     unsigned *inversions_per_vector_and_point);
/* Batch inversion and grand products over the scalar fields -- the step between "columns on the device" and "quotient on the coset": the
 * permutation (and lookup) argument's Z(w^0) = 1, Z(w^(i+1)) = Z(w^i) num_i / den_i, and the inverse of a whole vector (logUp denominators,
 * Lagrange and barycentric weights, the 1 / (X - zeta) columns of a batched opening).  field: 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr;
 * elements are the 32-byte Montgomery wire form of every other call.  Inputs are canonical residues, as every producer in this library
 * writes them; a non-canonical input is outside the contract.  Each vector costs ONE field inversion: with the identities
 *   1 / x_i = (prod_{j<i} x_j) (prod_{j>i} x_j) / prod_all x        Z_i = (prod_{j<i} num_j) (prod_{j>=i} den_j) / prod_all den
 * both calls are three kernel launches (tile totals; one workgroup per vector over the totals, which inverts; apply) and no kernel waits
 * for another workgroup.  The scratch (64 bytes per tile, 32 per vector) is the calling host thread's arena: a repeated call of the same
 * shape allocates nothing, panda_ntt_tear_down releases it.  It grows with batch x ceil(n / tile), not with batch x n: a batch of very
 * short vectors pays a tile's scratch, a workgroup of the second launch and one inversion per vector (n = 1, batch = 2^28 is legal and
 * asks for 16 GiB); the call is built for long vectors.
 *   panda_error_invalid_value, nothing launched, no output written: field > 2, n == 0, batch == 0, n or batch x n > 2^28, NULL d_in / d_out /
 *     d_num, a partial overlap (all checked before any runtime call), and buffers of this library's allocators shorter than stated. */
/* out[i] = in[i]^-1, and 0 where in[i] == 0.  n >= 1, n <= 2^28.  d_out == d_in exactly is legal (in place); any other overlap is refused.
 * Outputs canonical.  Synchronous on return.  Bytes behind the n elements are never written. */
panda_error panda_field_batch_inverse(unsigned field, const void *d_in, void *d_out, uint64_t n, panda_stream stream);
/* `batch` vectors of n elements, vector p at byte p * n * 32 of d_num, d_den and d_out:
 *   out[p][0] = 1,  out[p][i] = prod_{j < i} num[p][j] / den[p][j]  (i < n; n elements, the exclusive running product -- Z on the domain)
 *   totals[p] (HOST, batch x 32 B, may be NULL) = prod_{j < n} num[p][j] / den[p][j]  -- one for a valid permutation
 * d_den == NULL: the plain running product of num (no inversion of caller data; it costs what the full call costs).
 * A vector with a zero denominator anywhere: ALL n elements of out[p] and totals[p] are zero (out[p][0] == 0 is the signal); the other
 *   vectors of the batch are unaffected.  A zero numerator is ordinary arithmetic (zeros from the next index on, total zero).
 * d_out may equal d_num or d_den exactly (in place); d_num == d_den is legal; every other overlap among the three ranges is refused.
 * n >= 1 (any count, not only powers of two), batch >= 1, batch x n <= 2^28.  Outputs canonical.  Synchronous on return.  Bytes behind the
 * `batch` vectors are never written. */
panda_error panda_poly_grand_product(unsigned field, const void *d_num, const void *d_den, void *d_out, uint64_t n, unsigned batch,
                                     void *totals /* HOST, batch x 32 B, may be NULL */, panda_stream stream);
/* How the two calls run (pure host arithmetic, no device call): *tile_inverse / *tile_product = the elements one workgroup covers in the
 * inverse / the product kernels, *carry_chunk = the tile totals the second level takes per step, *launches = the kernel launches of either
 * call (the same for both).  None depends on `batch`.  Any pointer may be NULL.  Invalid for the shapes the execute calls refuse (n == 0,
 * batch == 0, n or batch x n > 2^28). */
panda_error panda_poly_product_plan(uint64_t n, unsigned batch, unsigned *tile_inverse, unsigned *tile_product, unsigned *carry_chunk, unsigned *launches);
/* Fused sum-of-products evaluation over device columns -- the "quotient on the coset" itself and every other element-wise polynomial
 * expression of a prover's round: the gate q_L a + q_R b + q_M a b + q_O c + q_C, the permutation check Z(wX) prod(..) - Z(X) prod(..),
 * Groth16's a b - c, each times the inverse of the vanishing polynomial; the fold sum_k v^k f_k in front of a batched opening; the
 * linearisation polynomial; the (a + beta id + gamma) factor columns panda_poly_grand_product takes.  For vector p < batch, index i < n:
 *   out[p][i] = s(p, i) * sum_{t < n_terms} coeff_t * prod_{f < degree_t} column[c_tf][p][(i + r_tf) mod n]
 * in ONE kernel launch and one pass over the columns; nothing intermediate goes to device memory.
 *   field: 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr.  Elements are the 32-byte Montgomery wire form of every other call; inputs are
 *     canonical residues, outputs are canonical.  n is ANY count from 1 up, batch >= 1, n and batch x n <= 2^28.
 *   columns: HOST array of n_columns DEVICE pointers, each to batch x n x 32 bytes, vector p at byte p x n x 32, read only.  Columns may
 *     be equal to each other or overlap each other freely (pointers into one extended buffer at different polynomials).
 *   coeffs (HOST, n_terms x 32 B), scales (HOST, n_scales x 32 B): wire elements below the modulus.  degrees (HOST, n_terms): the factor
 *     count of each term, 0 = a constant term.  factors (HOST, sum of the degrees, term after term): the column index and the rotation
 *     of each factor.  A rotation is any int32_t, reduced mod n on the host; it wraps inside vector p and never reaches vector p +- 1.
 *   scale_mode: PANDA_SOP_SCALE_NONE s = 1 (scales may be NULL); PANDA_SOP_SCALE_PER_VECTOR s = scales[p mod n_scales];
 *     PANDA_SOP_SCALE_CYCLIC s = scales[i mod n_scales].  With PANDA_NTT_LDE_COSET_MAJOR one extended polynomial is batch = B vectors
 *     of n, X -> wX is rotation +1 and 1 / Z_H is the constant 1 / (g^n w_N^(i n) - 1) on coset i: PER_VECTOR with n_scales = B.  With
 *     PANDA_NTT_LDE_NATURAL it is one vector of N, rotation +B, CYCLIC with n_scales = B.
 *   d_out (DEVICE, batch x n x 32 B) may equal a column's pointer exactly (in place) if and only if every factor on every column that
 *     overlaps d_out has a rotation that is 0 mod n; any partial overlap of d_out with a column is refused.
 *   Synchronous on return.  Bytes behind the `batch` vectors are never written.  The program (about 5 KB: pointers, reduced rotations,
 *     term offsets, coefficients and scales with the wire form's constants folded in) goes to the calling host thread's arena scratch: a
 *     repeated call allocates nothing, panda_ntt_tear_down releases it.
 *   panda_error_invalid_value, nothing launched, nothing written: field > 2, n == 0, batch == 0, n or batch x n > 2^28, NULL expr / d_out /
 *     columns / coeffs / degrees or a NULL column pointer, factors NULL while the degrees sum to more than 0, n_columns 0 or >
 *     PANDA_SOP_MAX_COLUMNS, n_terms 0 or > PANDA_SOP_MAX_TERMS, the degrees summing to more than PANDA_SOP_MAX_FACTORS, a factor's column
 *     index >= n_columns, scale_mode > 2, a scale mode other than NONE with scales NULL or n_scales 0 or > PANDA_SOP_MAX_SCALES, a
 *     coefficient or scale >= the modulus, the overlaps above (all checked before any runtime call), and buffers of this library's
 *     allocators shorter than stated. */
#define PANDA_SOP_MAX_COLUMNS 32
#define PANDA_SOP_MAX_TERMS   64
#define PANDA_SOP_MAX_FACTORS 256   /* sum of the terms' degrees */
#define PANDA_SOP_MAX_SCALES  16    /* 2^PANDA_NTT_LDE_MAX_LOG_BLOWUP */
#define PANDA_SOP_SCALE_NONE 0u
#define PANDA_SOP_SCALE_PER_VECTOR 1u   /* s = scales[p mod n_scales] */
#define PANDA_SOP_SCALE_CYCLIC 2u       /* s = scales[i mod n_scales] */
typedef struct panda_sop_factor { uint32_t column; int32_t rotation; } panda_sop_factor;
typedef struct panda_sop_expression {
    const void *const *columns;      /* HOST array of n_columns DEVICE pointers, each batch x n x 32 B, read only */
    const void *coeffs;              /* HOST, n_terms x 32 B, Montgomery wire form, value < modulus */
    const unsigned *degrees;         /* HOST, n_terms; 0 = a constant term */
    const panda_sop_factor *factors; /* HOST, sum(degrees) entries, term after term */
    const void *scales;              /* HOST, n_scales x 32 B, or NULL with SCALE_NONE */
    unsigned n_columns, n_terms, n_scales, scale_mode;
} panda_sop_expression;
panda_error panda_poly_sum_of_products(unsigned field, const panda_sop_expression *expr, void *d_out, uint64_t n, unsigned batch, panda_stream stream);
/* How the call runs (pure host arithmetic, no device call): *tile = the elements one workgroup covers, *launches = its kernel launches
 * (1).  Neither depends on `batch`.  Either pointer may be NULL.  Invalid for the shapes the call refuses (n == 0, batch == 0, n or
 * batch x n > 2^28). */
panda_error panda_poly_sum_of_products_plan(uint64_t n, unsigned batch, unsigned *tile, unsigned *launches);
/* logUp lookup support -- the two steps of a logarithmic-derivative lookup argument that are not arithmetic on columns.  The whole chain
 * stays on the device: panda_lookup_multiplicities (m) -> panda_poly_sum_of_products (alpha + f, alpha + t) -> panda_field_batch_inverse ->
 * panda_poly_sum_of_products (h_i = sum_k 1 / (alpha + f_k,i) - m_i / (alpha + t_i)) -> panda_poly_running_sum (Z, and the total that must
 * be zero).  field: 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr; elements are the 32-byte canonical Montgomery wire form of every other
 * call, a non-canonical input is outside the contract.
 *
 * Multiplicities.  Equality is equality of the 256-bit wire value; zero is an ordinary value.  With j0 the FIRST index at which a table
 * value occurs, d_mult[j0] is the wire form of the number of pairs (column c, index i) with columns[c][i] == table[j0], and d_mult[j] is
 * the wire zero for every later duplicate j of that value: sum_j m_j / (alpha + t_j) = sum 1 / (alpha + f) whatever the table repeats.
 *   *missing (HOST, may be NULL) = the number of pairs (c, i) whose value occurs nowhere in the table; *first_missing (HOST, may be NULL) =
 *     (c << 32) | i of the lexicographically smallest such pair, UINT64_MAX when there is none.  A missing value is data, not an error:
 *     the call still returns panda_success.
 *   Every output is deterministic: d_mult is byte for byte the same on every run.
 *   n_table >= 1, n >= 1, n_columns in 1..PANDA_LOOKUP_MAX_COLUMNS, n_table <= 2^28 and n_columns x n <= 2^28 (a count fits a u32 and one
 *     29-bit limb).  columns: HOST array of n_columns DEVICE pointers, n elements each.  Columns may be equal to each other, overlap each
 *     other and overlap the table; the table and the columns are read only; d_mult may overlap none of them.  Synchronous on return.
 *     Bytes behind d_mult's n_table elements are never written.
 *   The join is an open-addressing hash table of 2^log_slots >= 2 n_table slots (12 bytes each, and 4 bytes per table row) in the
 *     calling host thread's arena scratch: a repeated call of the same shape allocates nothing, panda_ntt_tear_down releases it.  Three
 *     kernel launches (build, probe, finish) on the caller's stream; no kernel waits for another workgroup.
 *   panda_error_invalid_value, nothing launched, no host output written: field > 2, n_table == 0 or > 2^28, n == 0, n or n_columns x n >
 *     2^28, n_columns 0 or > PANDA_LOOKUP_MAX_COLUMNS, NULL d_table / columns / d_mult or a NULL column pointer, d_mult overlapping the
 *     table or a column as address ranges (all checked before any runtime call), and buffers of this library's allocators shorter than
 *     stated. */
#define PANDA_LOOKUP_MAX_COLUMNS 32
panda_error panda_lookup_multiplicities(unsigned field, const void *d_table, uint64_t n_table,
                                        const void *const *columns /* HOST array of n_columns DEVICE pointers, n elements each */,
                                        unsigned n_columns, uint64_t n, void *d_mult /* DEVICE, n_table x 32 B */,
                                        uint64_t *missing /* HOST, may be NULL */, uint64_t *first_missing /* HOST, may be NULL */,
                                        panda_stream stream);
/* How the call runs (pure host arithmetic, no device call): *log_slots = log2 of the hash table's slot count (2^log_slots >= 2 n_table),
 * *scratch_bytes = the arena bytes the call reserves, *launches = its kernel launches, not counting memsets (3).  Any pointer may be
 * NULL.  Invalid for exactly the shapes the execute call refuses. */
panda_error panda_lookup_plan(uint64_t n_table, unsigned n_columns, uint64_t n, unsigned *log_slots, size_t *scratch_bytes, unsigned *launches);
/* The slot the library's hash gives a wire element (HOST, 32 B) in a table of 2^log_slots slots: where its walk starts (pure host
 * arithmetic; the kernels run the same code).  For tests that build collision chains and wrap-around cases on purpose.  Invalid for
 * field > 2, a NULL pointer, log_slots 0 or > 29. */
panda_error panda_lookup_home_slot(unsigned field, const void *elem /* HOST, 32 B */, unsigned log_slots, uint64_t *slot);
/* `batch` vectors of n elements, vector p at byte p * n * 32 of d_in and d_out:
 *   out[p][0] = 0,  out[p][i] = sum_{j < i} in[p][j]  (i < n; n elements, the exclusive running sum -- logUp's Z on the domain)
 *   totals[p] (HOST, batch x 32 B, may be NULL) = sum_{j < n} in[p][j]  -- zero for a valid logUp argument; asked for alone it is the
 *     plain sum of a vector (barycentric evaluation, every "does it sum to zero" check)
 * d_out == NULL computes the totals only and writes no device memory of the caller's; d_out and totals both NULL is refused.  d_out ==
 * d_in exactly is legal (in place); any other overlap is refused.  Any n >= 1, batch >= 1, batch x n <= 2^28.  Inputs canonical, outputs
 * canonical.  Synchronous on return.  Bytes behind the `batch` vectors are never written.  Three kernel launches (tile sums; one workgroup
 * per vector over the sums; apply), two for the totals alone; no kernel waits for another workgroup.  The scratch (32 bytes per tile and
 * per vector) is the calling host thread's arena.
 *   panda_error_invalid_value, nothing launched, no output written: field > 2, n == 0, batch == 0, n or batch x n > 2^28, NULL d_in, d_out
 *     and totals both NULL, a partial overlap (all checked before any runtime call), and buffers of this library's allocators shorter
 *     than stated. */
panda_error panda_poly_running_sum(unsigned field, const void *d_in, void *d_out /* may be NULL: totals only */, uint64_t n, unsigned batch,
                                   void *totals /* HOST, batch x 32 B, may be NULL */, panda_stream stream);
/* How the call runs (pure host arithmetic, no device call): *tile = the elements one workgroup covers, *carry_chunk = the tile sums the
 * second level takes per step, *launches_scan / *launches_total = the kernel launches with and without d_out (3, 2).  None depends on
 * `batch`.  Any pointer may be NULL.  Invalid for the shapes the execute call refuses (n == 0, batch == 0, n or batch x n > 2^28). */
panda_error panda_poly_running_sum_plan(uint64_t n, unsigned batch, unsigned *tile, unsigned *carry_chunk, unsigned *launches_scan, unsigned *launches_total);
/* Sumcheck over multilinear tables -- the round of HyperPlonk, Spartan, GKR, Lasso / Jolt and every zerocheck.  A table is 2^log_n
 * elements f[x], the values of a multilinear polynomial at the bits of x, in the 32-byte canonical Montgomery wire form of every other
 * call (field: 0 BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr); a non-canonical input is outside the contract.  A round binds one variable:
 *   PANDA_MLE_BIND_LOW   pair i < 2^(log_n - 1) is lo = f[2i], hi = f[2i + 1]            (arkworks fix_variables, HyperPlonk)
 *   PANDA_MLE_BIND_HIGH  pair i is lo = f[i], hi = f[i + 2^(log_n - 1)]                  (Spartan, Jolt, Lasso)
 *   fold with r:         F[i] = lo + r (hi - lo), 2^(log_n - 1) elements
 *   round polynomial:    g(t) = sum_i sum_terms coeff_term prod_{f < degree_term} ( lo_{c_f, i} + t (hi_{c_f, i} - lo_{c_f, i}) )
 * for t = 0 .. n_evals - 1, over the terms of a panda_sop_expression, the grammar of panda_poly_sum_of_products.
 *
 * panda_sumcheck_round.  expr: the columns are tables of 2^log_n elements (one vector each); every rotation must be 0 and scale_mode
 * PANDA_SOP_SCALE_NONE; the caps on columns, terms and factors are those of the sum of products.  n_evals in 1 ..
 * PANDA_SUMCHECK_MAX_EVALS: the caller asks for degree + 1 points, the library does not second-guess it.  evals[t] (HOST, n_evals x 32 B) =
 * g(t), canonical; field addition is exact, so the bytes are the same on every run whatever the order of the sums.
 *   challenge == NULL and folded == NULL: g over the tables as they stand, 2^(log_n - 1) pairs; log_n in 1 .. 28.  The columns are read
 *     only and may be equal to or overlap each other freely.
 *   challenge (HOST, 32 B, below the modulus) and folded (HOST array of n_columns DEVICE pointers, 2^(log_n - 1) elements each) both
 *     given, the FUSED round: every column is first folded with the challenge, in `order`, into folded[c], and g is taken over the folded
 *     tables, 2^(log_n - 2) pairs; log_n in 2 .. 28.  One pass: a thread reads the four source elements of a pair of folded elements,
 *     stores the two folded elements and evaluates from registers; nothing folded is read back.  Every column is folded, whether a
 *     factor names it or not.  Exactly one of the two pointers NULL is refused.
 *   A k-variable sumcheck is one plain round, k - 1 fused rounds (each with the challenge of the round before, log_n falling by one),
 *     and one panda_mle_fold on the 2-element tables, which gives the final evaluations.
 *   Aliasing (fused round and panda_mle_fold alike).  The folded ranges must be pairwise disjoint.  folded[c] == columns[c] exactly is in
 *     place, legal with PANDA_MLE_BIND_HIGH alone and only if columns[c] overlaps no other column: the thread of output i reads f[i] and
 *     f[i + half] and writes F[i] after it has read them, so it writes only bytes no other thread reads.  With PANDA_MLE_BIND_LOW output
 *     i lies where the thread of output i / 2 reads: in place is refused, as is every other overlap of a folded range with a column.
 *   Synchronous on return.  Two kernel launches (a sum per point and workgroup; one workgroup per point over those sums); no kernel waits
 *     for another workgroup, no atomics.  The program (about 7 KB) and n_evals x tiles x 32 bytes of sums go to the calling host
 *     thread's arena scratch: a repeated call allocates nothing, panda_ntt_tear_down releases it.  Bytes behind a folded table are never
 *     written.
 *   panda_error_invalid_value, nothing launched, no output written: field > 2, log_n outside the ranges above, order > 1, n_evals 0 or >
 *     PANDA_SUMCHECK_MAX_EVALS, NULL expr / evals / columns / coeffs / degrees, a NULL column or folded pointer, exactly one of challenge /
 *     folded NULL, the expression errors of panda_poly_sum_of_products (counts, a factor's column index), a rotation other than 0, a
 *     scale mode other than NONE, a coefficient or the challenge >= the modulus, the overlaps above (all checked before any runtime
 *     call), and buffers of this library's allocators shorter than stated.
 *
 * panda_mle_fold: the fold alone, folded[c][i] = lo + challenge (hi - lo) for all n_columns (1 .. PANDA_SOP_MAX_COLUMNS) tables in ONE
 * launch; log_n in 1 .. 28.  The last step of a sumcheck, and the unfused arm of a round.  Aliasing, refusals and synchronisation as above
 * (NULL columns / folded / challenge are refused).
 *
 * panda_mle_eq_table: d_out[x] = prod_{j < log_n} ( x_j r_j + (1 - x_j)(1 - r_j) ) for x < 2^log_n, x_j bit j of x and r_j = point[j]
 * (HOST, log_n x 32 B, each below the modulus) -- the table a zerocheck multiplies its gate by, and the weights of a multilinear
 * evaluation: sum_x f(x) eq(r, x) is g(0) + g(1) of the term f eq.  log_n in 0 .. 28; log_n = 0 writes the wire's one (point is then not
 * read but must not be NULL).  Canonical output, one launch, synchronous; the factors (about 2 KB) go to the arena scratch.  Refused:
 * field > 2, log_n > 28, NULL point / d_out, a coordinate >= the modulus, a d_out of this library's allocators shorter than stated.
 *
 * panda_sumcheck_plan (pure host arithmetic, no device call): *tile_pairs = the pairs one workgroup of the round kernel covers (`fused`
 * 0 / 1 selects the kernel), *carry_chunk = the tile sums the second level takes per step, *launches = the kernel launches of a round
 * (2).  Any pointer may be NULL.  Invalid for the shapes the round refuses: fused > 1, log_n < 1 + fused or > 28, n_evals 0 or above the
 * cap. */
#define PANDA_MLE_BIND_LOW  0u
#define PANDA_MLE_BIND_HIGH 1u
#define PANDA_SUMCHECK_MAX_EVALS 8   /* t = 0..7: degree 7, a degree-5 custom gate times eq fits */
panda_error panda_sumcheck_round(unsigned field, const panda_sop_expression *expr, unsigned log_n, unsigned order, unsigned n_evals,
                                 const void *challenge /* HOST 32 B, or NULL */, void *const *folded /* HOST array of n_columns DEVICE pointers, or NULL */,
                                 void *evals /* HOST, n_evals x 32 B */, panda_stream stream);
panda_error panda_mle_fold(unsigned field, const void *const *columns, void *const *folded, unsigned n_columns, unsigned log_n, unsigned order,
                           const void *challenge /* HOST 32 B */, panda_stream stream);
panda_error panda_mle_eq_table(unsigned field, const void *point /* HOST, log_n x 32 B */, unsigned log_n, void *d_out /* DEVICE 2^log_n x 32 B */, panda_stream stream);
panda_error panda_sumcheck_plan(unsigned log_n, unsigned fused, unsigned n_evals, unsigned *tile_pairs, unsigned *carry_chunk, unsigned *launches);
/* Sparse matrix-vector products over the scalar fields -- Az, Bz, Cz, the first step of every R1CS prover (Groth16, Marlin, Spartan), so
 * that the witness is the only upload and the columns of every later call are born on the device.  The matrix is CSR; field: 0 BN254 Fr,
 * 1 BLS12-377 Fr, 2 BLS12-381 Fr; elements are the 32-byte canonical Montgomery wire form of every other call, 16-byte aligned; a
 * non-canonical input is outside the contract.
 *
 * The product.  For p < batch and r < n_rows:  out[p][r] = sum_{k in row r} values[k] z[p][col[k]].  Vector p of d_z is at byte
 * p * n_cols * 32, vector p of d_out at byte p * n_rows * 32.  Outputs are canonical; an empty row gives the wire zero.  Field addition
 * is exact, so the bytes are identical on every run whatever the order of the sums.  Synchronous on return.
 *   Shapes: n_rows >= 1, n_cols >= 1, nnz >= 0 (nnz == 0 writes zeros; d_col and d_values may then be NULL), each <= 2^28; batch >= 1,
 *     batch x n_rows <= 2^28 and batch x n_cols <= 2^28.
 *   Aliasing: the matrix and d_z are read only and may overlap each other freely; d_out may overlap none of them, not even with exact
 *     equality (the gather reads all of z).  Bytes behind d_out's batch x n_rows elements are never written.
 *   The work is split by nonzeros, `tile` of them to a workgroup, so neither a row of millions of terms nor a run of millions of empty
 *     rows is a loop in any thread.  d_out is zeroed, then two kernel launches (the tiles; the rows that cross a tile end, none for a
 *     single tile); no kernel waits for another workgroup, no atomics on elements.  32 bytes per vector and tile go to the calling host
 *     thread's arena scratch: a repeated call of the same shape allocates nothing, panda_ntt_tear_down releases it.  (A shape of more
 *     than 2^31 - 1 vector-tiles, whose scratch alone is 64 GB, fails with the runtime's allocation error.)
 *   Memory safety: whatever bytes d_row_ptr and d_col hold, no kernel reads or writes outside the stated extents of the six buffers: a
 *     column index is compared with n_cols before it addresses z, a row index reaches d_out only below n_rows, a position reaches d_col
 *     and d_values only below nnz.  For a structure the check below would reject the VALUES of out are unspecified; the accesses are not.
 *   The transposed product is not offered (there is no atomic on a 256-bit residue): pass the CSR of the transpose.
 *   panda_error_invalid_value, nothing launched, nothing written: field > 2, the shapes above, a NULL m / d_row_ptr / d_z / d_out, a NULL
 *     d_col or d_values with nnz > 0, d_out overlapping any of the four inputs as address ranges, and buffers of this library's allocators
 *     shorter than stated -- all checked before any runtime call.
 *
 * The check.  One pass over the structure that dereferences nothing through an index and reports the FIRST defect, the smallest class
 * and then the smallest index (deterministic):  *defect = 0 none; 1 row_ptr[0] != 0; 2 row_ptr[r] > row_ptr[r + 1], *where = r;
 * 3 row_ptr[n_rows] != nnz; 4 col[k] >= n_cols, *where = k; 5 values[k] >= the modulus, *where = k.  *where is UINT64_MAX without a defect
 * and for the classes 1 and 3.  A defect is data: the call still returns panda_success.  Either out pointer may be NULL, not both.
 * One launch, synchronous, 8 bytes of arena scratch; refuses the shapes and matrix pointers the product refuses.
 *
 * The plan (pure host arithmetic, no device call): *tile = the nonzeros one workgroup covers, *carry_chunk = the tiles the second launch
 * adds per step and row, *scratch_bytes = the arena bytes, *launches = the kernel launches of the product, memsets not counted.  *tile
 * and *carry_chunk depend on none of the arguments.  Any pointer may be NULL.  Invalid for exactly the shapes the product refuses. */
typedef struct panda_csr_matrix
{
    const uint32_t *d_row_ptr; /* DEVICE, n_rows + 1 entries: row r holds the nonzeros row_ptr[r] .. row_ptr[r + 1] - 1 */
    const uint32_t *d_col;     /* DEVICE, nnz entries, each < n_cols; any order inside a row, repeats allowed (they add) */
    const void *d_values;      /* DEVICE, nnz x 32 B */
    uint64_t n_rows, n_cols, nnz;
} panda_csr_matrix;
panda_error panda_sparse_matvec(unsigned field, const panda_csr_matrix *m, const void *d_z /* DEVICE, batch x n_cols x 32 B */,
                                void *d_out /* DEVICE, batch x n_rows x 32 B */, unsigned batch, panda_stream stream);
panda_error panda_sparse_check(unsigned field, const panda_csr_matrix *m, unsigned *defect /* HOST, may be NULL */,
                               uint64_t *where /* HOST, may be NULL */, panda_stream stream);
panda_error panda_sparse_plan(uint64_t n_rows, uint64_t n_cols, uint64_t nnz, unsigned batch, unsigned *tile, unsigned *carry_chunk,
                              size_t *scratch_bytes, unsigned *launches);
/* The discrete Fourier transform over G1 points, and the batch conversion of result triples to affine points.  Both turn a vector of
 * points into a vector of points on the device: the first makes the Lagrange-basis SRS [L_i(tau)]G out of the monomial one (the inverse
 * transform: Q_i = n^-1 sum_j omega^(-ij) P_j) and is the core of amortised KZG openings, the second makes what panda_msm_execute_batch
 * returns fit for a transcript or for panda_msm_register_bases.  curve: 0 BN254, 1 BLS12-377, 2 BLS12-381, G1 only; the G2 ids (3, 4, 6)
 * are refused.  The reference has neither call.
 *
 * panda_ec_ntt.  out[k] = sum_j omega^(jk) P_j for k, j < n = 2^log_n, natural order in and out; PANDA_EC_NTT_INVERSE uses omega^-1 and
 * multiplies by n^-1, as panda_ntt_execute_*_inverse do.  `omega` is the FORWARD root for both directions: a HOST pointer to one
 * Montgomery-form scalar of 32 B, the convention of panda_ntt_configuration_v1.d_omega.  0 <= log_n <= PANDA_EC_NTT_MAX_LOG_N; log_n == 0
 * copies the point (omega is not read then, but must not be NULL).  Synchronous on return.
 *   Formats: d_in and d_out are n affine base points in the wire form the MSM takes, x || y, 64 B on BN254 and 96 B on the BLS curves,
 *     16-byte aligned.  x == 0 is the identity on input; on output the identity is all-zero bytes.  Output coordinates are canonical, so
 *     the bytes are the same on every run and the output can go straight to panda_msm_register_bases / panda_msm_precompute_bases.
 *   Aliasing: d_out == d_in exactly is in place and legal, any other overlap is refused.  Bytes behind d_out's n points are never
 *     written; d_in is unchanged by an out-of-place call.
 *   Scratch: the intermediate points (XYZZ, 144 B on BN254, 224 B on the BLS curves) and the table of the n / 2 canonical twiddles (32 B
 *     each, built on the device by every call) live in the calling host thread's arena: a repeated call of the same shape allocates
 *     nothing, panda_ntt_tear_down releases it.
 *   Invalid inputs: points off the curve or outside the prime-order subgroup, and non-canonical coordinates, are outside the contract:
 *     the VALUES are then unspecified, the memory accesses are not -- no index is ever derived from point data.
 *   The method is radix-2 over the points, one launch per stage; a multiplication by a twiddle is a double-and-add over its 256 bits.
 *     In the stages where at least 64 butterflies share a twiddle a wave runs 64 butterflies of one twiddle, so its bits are
 *     wave-uniform and a zero bit costs a doubling only; the other stages pay a doubling and an addition per bit.  P + P, P + (-P) and
 *     the identity take the exact paths of the group law.  No kernel waits for another workgroup; there are no atomics.
 *   panda_error_invalid_value, nothing launched, nothing written: curve > 2, log_n > PANDA_EC_NTT_MAX_LOG_N, direction > 1, a NULL d_in /
 *     d_out / omega, for log_n >= 1 an omega >= the modulus or with omega^(2^(log_n - 1)) != -1 (not a primitive 2^log_n-th root), the
 *     overlaps above, and buffers of this library's allocators shorter than stated -- all checked before any runtime call.
 *   The plan (pure host arithmetic): *launches = the kernel launches of the call, *scratch_bytes = its arena bytes, *uniform_stages = the
 *     stages in which every wave's butterflies share one twiddle (the first, which multiplies by nothing, included).  Any pointer may be
 *     NULL.  Invalid for curve > 2, log_n > the cap, direction > 1.
 *
 * panda_points_to_affine.  d_in holds n points as X || Y || Z triples in the MSM result form (96 B on BN254, 144 B on the BLS curves;
 * JACOBIAN x = X / Z^2, y = Y / Z^3 or PROJECTIVE x = X / Z, y = Y / Z by in_type; identity <=> Z == 0), d_out receives n affine wire
 * points, canonical, the identity as all-zero bytes.  1 <= n <= 2^28.  One launch, no scratch, synchronous on return: a thread takes
 * `chunk` consecutive points, forms the prefix products of their Z (skipping identities; the products are parked in the output slots),
 * inverts once and walks back.  The last chunk is short; a chunk of identities alone inverts nothing.
 *   Aliasing: any overlap of the two buffers is refused.  d_in is unchanged; bytes behind d_out's n points are never written.
 *   panda_error_invalid_value, nothing launched, nothing written: curve > 2, an in_type that is neither, n == 0 or n > 2^28, a NULL
 *     pointer, overlapping buffers, buffers of this library's allocators shorter than stated -- all checked before any runtime call.
 *   The plan: *chunk = the points per inversion (it depends on nothing), *launches = 1.  Either pointer may be NULL.  Invalid for n == 0
 *     and n > 2^28. */
#define PANDA_EC_NTT_FORWARD 0u
#define PANDA_EC_NTT_INVERSE 1u   /* omega^-1 and the n^-1 scaling, as panda_ntt_execute_*_inverse */
#define PANDA_EC_NTT_MAX_LOG_N 26 /* the MSM's own cap: a larger base set has no consumer */
panda_error panda_ec_ntt(unsigned curve, const void *d_in, void *d_out, unsigned log_n, unsigned direction,
                         const void *omega /* HOST, 32 B */, panda_stream stream);
panda_error panda_ec_ntt_plan(unsigned curve, unsigned log_n, unsigned direction, unsigned *launches, size_t *scratch_bytes,
                              unsigned *uniform_stages);
panda_error panda_points_to_affine(unsigned curve, const void *d_in, panda_msm_result_coordinate_type in_type, void *d_out, uint64_t n,
                                   panda_stream stream);
panda_error panda_points_to_affine_plan(uint64_t n, unsigned *chunk, unsigned *launches);
/* Element-wise scalar multiplication of a vector of G1 points, and with it the KZG proofs of one polynomial at ALL points of its domain
 * (Feist-Khovratovich).  curve: 0 BN254, 1 BLS12-377, 2 BLS12-381, G1 only; the G2 ids (3, 4, 6) are refused.  The reference has neither.
 *
 * panda_points_scalar_mul.  out[i] = A_i + k_i P_i for i < n, 1 <= n <= 2^28; the A_i term is omitted when d_addend is NULL.
 *   mode PANDA_POINTS_MUL_EACH:   k_i = d_scalars[i] (DEVICE, n x 32 B); h_scalars must be NULL.  The FK20 product, folds of commitments.
 *   mode PANDA_POINTS_MUL_ONE:    k_i = the one scalar at h_scalars (HOST, 32 B); d_scalars must be NULL.  The IPA fold, blinding.
 *   mode PANDA_POINTS_MUL_POWERS: k_i = c s^i with (c, s) at h_scalars (HOST, 64 B); d_scalars must be NULL.  A powers-of-tau update,
 *     the coset shift of a Lagrange SRS.
 *   Formats: d_points, d_addend and d_out are n affine points in the wire form the MSM takes (x || y, 64 B on BN254, 96 B on the BLS
 *     curves, 16-byte aligned); x == 0 is the identity on input, on output the identity is all-zero bytes and coordinates are canonical.
 *     Scalars are 32-byte Montgomery-form residues of the curve's Fr, as in every other call.  Synchronous on return.
 *   Aliasing: d_out is written by the second launch only, after every input has been read, so d_out == d_points or d_out == d_addend
 *     exactly is legal; any other overlap among d_points, d_addend and d_out is refused.  Inputs of an out-of-place call are unchanged;
 *     bytes behind d_out's n points are never written.
 *   Method: two launches.  The first forms k_i P_i by left-to-right double-and-add, adds A_i and writes an XYZZ point (144 B on BN254,
 *     224 B on the BLS curves) to the calling host thread's arena (a repeated call of the same shape allocates nothing,
 *     panda_ntt_tear_down releases it); the second is the batch normalisation of panda_ec_ntt.  The loop runs over the longest scalar
 *     of a wave of 64 points, not over 256 bits: a vector of 128-bit challenges costs 128 steps.  In ONE mode every branch on the
 *     scalar is wave-uniform and a zero bit costs a doubling only; in the other modes a wave pays the doubling and the addition for
 *     every step.  k_i = 0, P_i the identity, A_i = -k_i P_i and A_i = k_i P_i take the exact paths of the group law.
 *   Invalid inputs: points off the curve, non-canonical coordinates and a DEVICE scalar at or above the modulus are outside the
 *     contract: the values are then unspecified, the memory accesses are not -- no index is derived from point or scalar data.
 *   panda_error_invalid_value, nothing launched, nothing written: curve > 2, mode > 2, n == 0 or n > 2^28, a NULL d_points / d_out, the
 *     scalar pointer of the chosen mode NULL or the pointer of the other kind non-NULL, a host scalar >= the modulus, the overlaps above,
 *     and buffers of this library's allocators shorter than stated -- all checked before any runtime call.
 *   The plan (pure host arithmetic): *launches = 2, *scratch_bytes = n x the XYZZ point rounded up to 256, plus 256.  Either pointer may
 *     be NULL.  Invalid for the shapes the call refuses.
 *
 * panda_kzg_open_all.  d_proofs[k] = the commitment to (f(X) - f(w^k)) / (X - w^k) under the SRS s_i = [tau^i]G, for all k < n = 2^log_n,
 * 1 <= log_n <= PANDA_KZG_OPEN_ALL_MAX_LOG_N, w = omega2^2.  `omega2` is a HOST pointer to one Montgomery-form scalar (32 B): a primitive
 * 2n-th root of unity, in the convention of panda_ec_ntt's omega and checked the same way.  With h_m = sum_{i <= n-2-m} f_(m+1+i) s_i
 * (h_(n-1) the identity) the proofs are the EC-DFT of h, and h_m is entry n - 1 + m of the linear convolution of f with the reversed SRS
 * s'_j = s_(n-2-j): 2n - 2 entries, so a cyclic convolution of length 2n does not wrap.
 *   panda_kzg_open_all_setup: d_table (2n points) = the forward EC-NTT of size 2n of (s'_0 .. s'_(n-2), n + 1 identities): one copy kernel
 *     and panda_ec_ntt in place.  Once per SRS and size.  d_srs (n points) is not modified; d_table must not overlap it.
 *   panda_kzg_open_all: d_coeffs (n scalars) padded with n zeros into d_work; panda_ntt_execute_batch forward at size 2n (one member);
 *     panda_points_scalar_mul EACH against d_table; panda_ec_ntt inverse at size 2n; entries n - 1 .. 2n - 3 and one identity into
 *     d_proofs; panda_ec_ntt forward at size n with omega2^2 in place in d_proofs.  About 2n log 2n + n log n scalar multiplications of
 *     points in place of n MSMs of size n.  Synchronous on return.  d_coeffs and d_table are unchanged; bytes behind the n proofs are
 *     never written.  Proofs are affine wire points, canonical, the identity as all-zero bytes.
 *   Workspace: d_work holds the temporaries (the parts take the calling thread's arena themselves): *work_bytes of the plan = 2n x 32 B +
 *     2n x point bytes, rounded up to 256.  Its contents after a call are unspecified.
 *   panda_error_invalid_value, nothing launched, nothing written: as for the parts, and: log_n == 0 or > the cap, a NULL pointer, an
 *     omega2 >= the modulus or with omega2^n != -1, work_bytes below the plan's, any overlap among d_coeffs, d_table, d_work and d_proofs
 *     (setup: between d_srs and d_table), buffers of this library's allocators shorter than stated -- all before any runtime call.
 *   The plan: *launches = 1 (pad) + the passes of the scalar transform (panda_ntt_batch_plan at log_n + 1) + panda_points_scalar_mul_plan's
 *     + panda_ec_ntt_plan's at (log_n + 1, inverse) + 1 (the middle copy) + panda_ec_ntt_plan's at (log_n, forward).  Either pointer may
 *     be NULL.  Invalid for curve > 2, log_n == 0 and log_n > the cap. */
#define PANDA_POINTS_MUL_EACH 0u
#define PANDA_POINTS_MUL_ONE 1u
#define PANDA_POINTS_MUL_POWERS 2u
#define PANDA_KZG_OPEN_ALL_MAX_LOG_N 25 /* 2n within PANDA_EC_NTT_MAX_LOG_N */
panda_error panda_points_scalar_mul(unsigned curve, unsigned mode, const void *d_points, const void *d_scalars /* DEVICE, mode EACH */,
                                    const void *h_scalars /* HOST, modes ONE (32 B) and POWERS (64 B: c, s) */,
                                    const void *d_addend /* DEVICE, may be NULL */, void *d_out, uint64_t n, panda_stream stream);
panda_error panda_points_scalar_mul_plan(unsigned curve, unsigned mode, uint64_t n, unsigned *launches, size_t *scratch_bytes);
panda_error panda_kzg_open_all_setup(unsigned curve, const void *d_srs /* n points [tau^i]G */, unsigned log_n, const void *omega2 /* HOST, 32 B */,
                                     void *d_table /* 2n points */, panda_stream stream);
panda_error panda_kzg_open_all(unsigned curve, const void *d_coeffs /* n scalars */, const void *d_table, unsigned log_n, const void *omega2,
                               void *d_work, size_t work_bytes, void *d_proofs /* n points */, panda_stream stream);
panda_error panda_kzg_open_all_plan(unsigned curve, unsigned log_n, size_t *work_bytes, unsigned *launches);
/* Poseidon over the scalar fields: the permutation, a sponge hash and a Merkle tree over device-resident elements, so that a transcript,
 * a witness generator's tree of 2^20 .. 2^24 leaves or the commitment to the rows of a low-degree extension needs no download.  field: 0
 * BN254 Fr, 1 BLS12-377 Fr, 2 BLS12-381 Fr; elements are the 32-byte canonical Montgomery wire form of every other call, 16-byte aligned;
 * a non-canonical DEVICE input is outside the contract (the values are then unspecified, the accesses are not).  The reference has none
 * of these calls.
 *
 * The permutation on a state of t = width elements.  Each of the R_F + R_P rounds adds the round's t constants, applies x -> x^alpha to
 * every element (a full round: the first and the last R_F / 2) or to state[0] alone (a partial round), and multiplies by the matrix:
 * new[i] = sum_j mds[i][j] old[j].  This is the plain definition and the one circomlib's poseidon computes.  Results are canonical, byte
 * for byte the same on every run.  The library does not check that the matrix is MDS: that is the caller's parameter set.
 *
 * panda_poseidon_create validates the parameters, derives the device table -- the constants as (w, floor(w R / p)) pairs with the wire
 * form's factors folded in -- and allocates it with panda_malloc; the host arrays may be freed when it returns.  panda_poseidon_destroy
 * gives the table back.  A handle belongs to the device that was current at its creation.
 *
 * panda_poseidon_permute: n states of t contiguous elements, 1 <= n <= 2^28.  d_out == d_in exactly is in place, any other overlap is
 * refused.
 *
 * panda_poseidon_hash: n messages of len >= 1 elements, one thread each, n x len <= 2^28.  Element j of message i is at d_in + 32 (i
 * msg_stride + j elem_stride), strides in elements, each <= 2^28: (len, 1) is contiguous messages, (1, n) is row i across len column
 * vectors of n elements -- the layout panda_ntt_execute_batch and panda_ntt_execute_lde leave, whose loads coalesce.  The state starts as
 * (tag, 0, .., 0); each chunk of t - 1 elements is added into state[1 ..], the last one zero-padded (encode the length in `tag` if
 * needed), and the state is permuted after every chunk; d_out[i] is state[0] after the last.  With len <= t - 1 and tag = 0 this is
 * circomlib's hash.  d_out (n elements) must not overlap the input extent, (n - 1) msg_stride + (len - 1) elem_stride + 1 elements.
 *
 * panda_poseidon_merkle_tree: arity a = t - 1 >= 2 (width 2 is refused), n = a^height leaves, height >= 1, n <= 2^28.  d_nodes takes the
 * (n - 1) / (a - 1) inner nodes level by level from the bottom: level 1 is n / a nodes at offset 0, the root is last;
 * node = permute: (tag, child_0 .. child_(a-1)), element 0 -- every level is panda_poseidon_hash over the level below with len = a.
 * `root` (HOST, 32 B, may be NULL) receives the last node.  d_nodes must not overlap d_leaves.  One launch per level while a level has
 * more than *per_workgroup nodes, then ONE single-workgroup launch for the *top_levels levels above, with a workgroup barrier between two
 * levels: a tree of 24 levels is 16 launches, not 24.  No kernel waits for another workgroup; no atomics, no flags.
 *
 * panda_poseidon_plan (pure host arithmetic): *per_workgroup = the permutations one workgroup covers (it depends on nothing), *nodes =
 * the node count, level_offset[l - 1] = the element offset of level l = 1 .. height in d_nodes (height entries; an authentication path
 * reads node (index / a^l) of level l), *top_levels and *launches as above.  Any pointer may be NULL.  Invalid for width < 3, width >
 * PANDA_POSEIDON_MAX_WIDTH, height == 0 and more than 2^28 leaves.
 *
 * All calls but the plan are synchronous on return.  panda_error_invalid_value, nothing launched, nothing written: field > 2, the
 * parameter ranges in the struct below, a round constant, matrix entry or tag >= the modulus, an alpha that divides p - 1, the shapes
 * above, a NULL pointer (but `root`), a NULL or destroyed handle, the overlaps above, and buffers of this library's allocators shorter
 * than stated -- all checked before any runtime call.  No kernel reads or writes outside the stated extents. */
#define PANDA_POSEIDON_MAX_WIDTH 5
typedef struct panda_poseidon_params
{
    unsigned width;              /* t = rate + 1, 2 .. PANDA_POSEIDON_MAX_WIDTH; state[0] is the capacity element */
    unsigned alpha;              /* S-box x^alpha: 5, 7, 11 or 17, and alpha must not divide p - 1 */
    unsigned full_rounds;        /* R_F, even, 2 .. 16: R_F / 2 before and R_F / 2 after the partial rounds */
    unsigned partial_rounds;     /* R_P, 0 .. 128: S-box on state[0] only */
    const void *round_constants; /* HOST, (R_F + R_P) x t x 32 B, round-major, wire form, each < modulus */
    const void *mds;             /* HOST, t x t x 32 B, row-major, wire form: new[i] = sum_j mds[i][j] old[j] */
} panda_poseidon_params;
typedef struct panda_poseidon { void *handle; } panda_poseidon; /* as panda_multi_gpu */
panda_error panda_poseidon_create(unsigned field, const panda_poseidon_params *params, panda_poseidon *out);
panda_error panda_poseidon_destroy(panda_poseidon p);
panda_error panda_poseidon_permute(panda_poseidon p, const void *d_in, void *d_out, uint64_t n, panda_stream stream);
panda_error panda_poseidon_hash(panda_poseidon p, const void *d_in, uint64_t len, uint64_t msg_stride, uint64_t elem_stride,
                                const void *tag /* HOST, 32 B */, void *d_out, uint64_t n, panda_stream stream);
panda_error panda_poseidon_merkle_tree(panda_poseidon p, const void *d_leaves, unsigned height, const void *tag /* HOST, 32 B */,
                                       void *d_nodes, void *root /* HOST, 32 B, may be NULL */, panda_stream stream);
panda_error panda_poseidon_plan(unsigned width, unsigned height, unsigned *per_workgroup, uint64_t *nodes,
                                uint64_t *level_offset /* height entries, may be NULL */, unsigned *top_levels, unsigned *launches);
/* Clock stamps (measurement only; off by default).  With panda_set_clock_stamps(1) an MSM brackets the k_accumulate launch of its last
 * range, and a whole NTT its passes, with a marker kernel in which one wave per CU stores s_memtime (shader cycles) and s_memrealtime
 * (100 MHz); stamps are only compared within one CU (the cycle counter is not chip-wide).  panda_*_last_clock fills PANDA_CLOCK_WORDS u64:
 *   [0] shader cycles of the XCD that showed the fewest -- the slowest-clocked one, which the launch waits for (the faster XCDs idle at
 *       the end of a launch and show more): the cycles the CODE needed
 *   [1] 10 ns ticks (median over the CUs)      [2] XCDs stamped on both sides      [3] mean of the XCDs' cycles: what rocprofv3's
 *       GRBM_GUI_ACTIVE / 8 shows for the same launch; [3] / [1] x 100 MHz is the clock the BOX held     [4..11] cycles per XCD
 * A record with cycles and MHz tells a slower kernel from a slower device.  panda_clock_stamp enqueues one marker on `stream` into a
 * block of PANDA_CLOCK_STAMP_BYTES the device can write (clear it first); panda_clock_delta reduces two blocks (host copies) the same way. */
#define PANDA_CLOCK_WORDS 12
#define PANDA_CLOCK_STAMP_BYTES 32768
panda_error panda_set_clock_stamps(unsigned on);
panda_error panda_msm_last_clock(uint64_t *out /* PANDA_CLOCK_WORDS */);
panda_error panda_ntt_last_clock(uint64_t *out /* PANDA_CLOCK_WORDS */);
panda_error panda_clock_stamp(panda_stream stream, void *block /* PANDA_CLOCK_STAMP_BYTES */);
panda_error panda_clock_delta(const void *before, const void *after, uint64_t *out /* PANDA_CLOCK_WORDS */);
/* Bit-reversed orderings (SURVEY 8f-4 "bit-reversed NTT variants"): the forward transform with y[k] stored at bitrev(k), and the inverse
 * (n^-1 fused) of a buffer in that order back to natural-order coefficients.  Chaining them skips two permutations. */
panda_error panda_ntt_execute_bn254_bitrev_out(const panda_ntt_configuration_v1 exec_cfg);
panda_error panda_ntt_execute_bn254_inverse_bitrev_in(const panda_ntt_configuration_v1 exec_cfg);
/* Coset transforms (additive): forward y[k] = sum_j x[j] g^j w^(jk), inverse x[j] = g^-j n^-1 sum_k y[k] w^(-jk); `shift` is a HOST pointer
 * to g in Montgomery form (32 bytes, non-zero), d_omega the forward root as for _v1.  In place on d_src/d_dst with the usual flag protocol. */
panda_error panda_ntt_execute_bn254_coset(const panda_ntt_configuration_v1 exec_cfg, const void *shift);
panda_error panda_ntt_execute_bn254_coset_inverse(const panda_ntt_configuration_v1 exec_cfg, const void *shift);
/* The same transforms over the BLS12-377 scalar field (README.md:36: "easy to encapsulate ... BLS12-377 later") */
panda_error panda_ntt_execute_bls12_377_v1(const panda_ntt_configuration_v1 exec_cfg);
panda_error panda_ntt_execute_bls12_377_inverse(const panda_ntt_configuration_v1 exec_cfg);
/* ... in every variant the BN254 field has (north_star: "NTT butterfly over BN254/BLS12-377"; field parameters:
 * src/cuda/core/curve/bls12_377/paramter.cuh:130-181): bit-reversed orderings and coset transforms, semantics as for the _bn254_ entry points */
panda_error panda_ntt_execute_bls12_377_bitrev_out(const panda_ntt_configuration_v1 exec_cfg);
panda_error panda_ntt_execute_bls12_377_inverse_bitrev_in(const panda_ntt_configuration_v1 exec_cfg);
panda_error panda_ntt_execute_bls12_377_coset(const panda_ntt_configuration_v1 exec_cfg, const void *shift);
panda_error panda_ntt_execute_bls12_377_coset_inverse(const panda_ntt_configuration_v1 exec_cfg, const void *shift);
panda_error panda_ntt_execute_bls12_381_v1(const panda_ntt_configuration_v1 exec_cfg);
panda_error panda_ntt_execute_bls12_381_inverse(const panda_ntt_configuration_v1 exec_cfg);
panda_error panda_ntt_execute_bls12_381_bitrev_out(const panda_ntt_configuration_v1 exec_cfg);
panda_error panda_ntt_execute_bls12_381_inverse_bitrev_in(const panda_ntt_configuration_v1 exec_cfg);
panda_error panda_ntt_execute_bls12_381_coset(const panda_ntt_configuration_v1 exec_cfg, const void *shift);
panda_error panda_ntt_execute_bls12_381_coset_inverse(const panda_ntt_configuration_v1 exec_cfg, const void *shift);

/* Multi-GPU, one process per GPU.  The exchange itself is the caller's (RCCL through
 * torch.distributed or ncclAllGather): these are the per-rank halves either side of it.
 *   MSM  : each rank runs panda_msm_execute_* on its base range -> one partial (96/144 B);
 *          after the all-gather of partials every rank (or rank 0) calls panda_msm_combine_*.
 *   NTT  : four-step over `ranks` slabs; see DESIGN.md section "multi-GPU". */
panda_error panda_msm_combine_bn254(const void *partials /* host or device, count x 96 B Jacobian */, unsigned count,
                                    panda_msm_result_coordinate_type out_type, void *result /* host, 96 B */);
panda_error panda_msm_combine_bls12_377(const void *partials, unsigned count, panda_msm_result_coordinate_type out_type, void *result);
panda_error panda_msm_combine_bls12_381(const void *partials, unsigned count, panda_msm_result_coordinate_type out_type, void *result);

typedef struct panda_ntt_slab_configuration
{
    panda_stream stream;
    void *d_slab;    /* device: this rank's rows, (n / ranks) elements */
    void *d_scratch; /* device: same size */
    void *omega;     /* HOST pointer: primitive n-th root, Montgomery form */
    unsigned log_n;  /* global size */
    unsigned log_ranks;
    unsigned rank;
    void *flag;      /* host unsigned*: which of d_slab / d_scratch holds the step's output */
} panda_ntt_slab_configuration;
/* step 1: local column transforms + inter-slab twiddle; step 2 (after the all-to-all): local row transforms */
panda_error panda_ntt_slab_step1_bn254(const panda_ntt_slab_configuration cfg);
panda_error panda_ntt_slab_step2_bn254(const panda_ntt_slab_configuration cfg);
/* the same steps, enqueued on cfg.stream without waiting (flag is valid on return): step 1 -> all-to-all -> step 2 on one stream needs one
 * synchronisation at the end */
panda_error panda_ntt_slab_step1_bn254_enqueue(const panda_ntt_slab_configuration cfg);
panda_error panda_ntt_slab_step2_bn254_enqueue(const panda_ntt_slab_configuration cfg);
/* The inverse of the sharded transform, from the forward transform's output layout back to its input layout (n^-1 included), by the
 * mirrored steps: inverse_step1 (size-G inverse transforms) -> the same all-to-all -> inverse_step2 (twiddle w^(-r k2) / n, then the local
 * inverse transform).  cfg.omega is the FORWARD root.  Enqueued without waiting, flag valid on return. */
panda_error panda_ntt_slab_inverse_step1_bn254_enqueue(const panda_ntt_slab_configuration cfg);
panda_error panda_ntt_slab_inverse_step2_bn254_enqueue(const panda_ntt_slab_configuration cfg);
/* the four enqueued halves over the BLS12-377 scalar field */
panda_error panda_ntt_slab_step1_bls12_377_enqueue(const panda_ntt_slab_configuration cfg);
panda_error panda_ntt_slab_step2_bls12_377_enqueue(const panda_ntt_slab_configuration cfg);
panda_error panda_ntt_slab_inverse_step1_bls12_377_enqueue(const panda_ntt_slab_configuration cfg);
panda_error panda_ntt_slab_inverse_step2_bls12_377_enqueue(const panda_ntt_slab_configuration cfg);
/* ... and over the BLS12-381 scalar field */
panda_error panda_ntt_slab_step1_bls12_381_enqueue(const panda_ntt_slab_configuration cfg);
panda_error panda_ntt_slab_step2_bls12_381_enqueue(const panda_ntt_slab_configuration cfg);
panda_error panda_ntt_slab_inverse_step1_bls12_381_enqueue(const panda_ntt_slab_configuration cfg);
panda_error panda_ntt_slab_inverse_step2_bls12_381_enqueue(const panda_ntt_slab_configuration cfg);

/* Multi-GPU, ONE process (no reference counterpart: msm_cuda.cuh:554-555 pins device 0, wrapper.rs:38 opens one
 * device, binding.rs:54-56 only declares the peer-access symbols).  A panda_multi_gpu owns one host thread, one stream and -- with
 * PANDA_MULTI_RCCL -- one RCCL communicator per device (ncclCommInitAll); the whole sharded operation is one call:
 *   panda_msm_execute_*_multi   cfgs[d] is an ordinary panda_msm_configuration whose buffers live on devices[d] and describe that
 *                               device's base-point range (stream.handle == NULL: the handle's own stream of that device).  Every device
 *                               runs the single-GPU pipeline on its worker thread and leaves its JACOBIAN partial in cfgs[d].results;
 *                               one ncclAllGather moves the partials, the sum in cfgs[0]'s coordinate type goes to `result` (HOST, 96 /
 *                               144 bytes).  Synchronous on return.
 *   panda_ntt_execute_*_multi   cfgs[d] is the slab configuration of rank d (rank == d, log_ranks == log2(n_dev), a power of two):
 *                               step 1 on every device, ONE grouped ncclSend / ncclRecv all-to-all (chunk q of rank d to rank q), step 2
 *                               on every device, one synchronisation at the end.  *cfgs[d].flag (HOST) = 1 if rank d's output sits in
 *                               its d_scratch, 0 if in its d_slab.  Layouts as for the panda_ntt_slab_* halves above.
 * PANDA_MULTI_LOOPBACK replaces RCCL by device-to-device copies and lets one device play several ranks (tests on a one-GPU box; also
 * what a caller without xGMI peers gets).  The worker threads keep the library's per-thread scratch and twiddle caches alive between
 * calls; per-device setup (allocation, panda_msm_precompute_bases) is done by the caller under panda_set_device(devices[d]). */
typedef struct panda_multi_gpu { void *handle; } panda_multi_gpu;
#define PANDA_MULTI_RCCL 0u
#define PANDA_MULTI_LOOPBACK 1u
panda_error panda_multi_gpu_create(panda_multi_gpu *out, const int *devices, unsigned n_dev, unsigned transport);
panda_error panda_multi_gpu_destroy(panda_multi_gpu mg);
panda_error panda_multi_gpu_device_count(panda_multi_gpu mg, unsigned *n_dev);
panda_error panda_msm_execute_bn254_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs /* n_dev */, void *result /* host */);
panda_error panda_msm_execute_bls12_377_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, void *result);
panda_error panda_msm_execute_bls12_381_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, void *result /* 144 B */);
panda_error panda_msm_execute_bn254_g2_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, void *result /* 192 B */);
panda_error panda_msm_execute_bls12_381_g2_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, void *result /* 288 B */);
panda_error panda_msm_execute_bls12_377_g2_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, void *result /* 288 B */);
/* The same with the scalars starting on the HOST ("scalars H2D'd per shard"; replaces the staging of unit.rs:103-188, which
 * uploads before it executes): h_scalars[d] is rank d's host source (pinned memory lets the copies run beside the kernels, pageable
 * memory works), cfgs[d].scalars the device buffer it lands in.  Every device's worker runs panda_msm_execute_from_host on its shard --
 * `ranges` point ranges, upload of range r+1 beside the kernels of range r, on the device's own copy stream and PCIe link -- so the
 * n_dev uploads run side by side; then the one ncclAllGather and the combine as above. */
panda_error panda_msm_execute_bn254_from_host_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs /* n_dev */, const void *const *h_scalars /* n_dev */,
                                                    unsigned ranges, void *result /* host */);
panda_error panda_msm_execute_bls12_377_from_host_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, const void *const *h_scalars, unsigned ranges,
                                                        void *result);
panda_error panda_msm_execute_bls12_381_from_host_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, const void *const *h_scalars, unsigned ranges,
                                                        void *result);
panda_error panda_msm_execute_bn254_g2_from_host_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, const void *const *h_scalars, unsigned ranges,
                                                       void *result);
panda_error panda_msm_execute_bls12_381_g2_from_host_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, const void *const *h_scalars, unsigned ranges,
                                                           void *result);
panda_error panda_msm_execute_bls12_377_g2_from_host_multi(panda_multi_gpu mg, const panda_msm_configuration *cfgs, const void *const *h_scalars, unsigned ranges,
                                                           void *result);
panda_error panda_ntt_execute_bn254_multi(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs /* n_dev */);
panda_error panda_ntt_execute_bn254_inverse_multi(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs);
/* A batch of `count` sharded transforms (same size and root; cfgs[t * n_dev + d] = rank d of transform t, every transform with its own slab and
 * scratch) pipelined over two streams per device: the all-to-all of transform t runs while step 1 of transform t + 1 and step 2 of transform
 * t - 1 compute.  Layouts, flags and results as `count` separate panda_ntt_execute_bn254[_inverse]_multi calls; one synchronisation at the end. */
panda_error panda_ntt_execute_bn254_multi_batch(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs /* count x n_dev */, unsigned count);
panda_error panda_ntt_execute_bn254_inverse_multi_batch(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs, unsigned count);
/* the sharded transforms over the BLS12-377 scalar field */
panda_error panda_ntt_execute_bls12_377_multi(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs /* n_dev */);
panda_error panda_ntt_execute_bls12_377_inverse_multi(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs);
panda_error panda_ntt_execute_bls12_377_multi_batch(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs /* count x n_dev */, unsigned count);
panda_error panda_ntt_execute_bls12_377_inverse_multi_batch(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs, unsigned count);
panda_error panda_ntt_execute_bls12_381_multi(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs /* n_dev */);
panda_error panda_ntt_execute_bls12_381_inverse_multi(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs);
panda_error panda_ntt_execute_bls12_381_multi_batch(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs /* count x n_dev */, unsigned count);
panda_error panda_ntt_execute_bls12_381_inverse_multi_batch(panda_multi_gpu mg, const panda_ntt_slab_configuration *cfgs, unsigned count);
/* per-phase device times of rank's last MSM inside a *_multi call (the workers' panda_msm_last_phase_ms) */
panda_error panda_multi_gpu_last_phase_ms(panda_multi_gpu mg, unsigned rank, float *ms /* PANDA_MSM_PHASES floats */);

/* Synthetic inputs generated on the device; curve: 0 = BN254, 1 = BLS12-377, 2 = BLS12-381, 3 = BN254 G2, 4 = BLS12-381 G2,
 * 6 = BLS12-377 G2 */
panda_error panda_gen_scalars(unsigned curve, uint64_t seed, uint64_t first, uint64_t n, void *d_out, panda_stream stream);
panda_error panda_gen_bases(unsigned curve, uint64_t seed, uint64_t first, uint64_t n, void *d_out, panda_stream stream);

/* Element-wise diagnostics used by the parity tests: field id 0..5 = BN254 Fq, BN254 Fr, BLS12-377 Fq, BLS12-377 Fr, BLS12-381 Fq, BLS12-381 Fr;
 * op 0..6 = add, sub, mul, sqr, to_montgomery, from_montgomery, inverse (Montgomery in/out, 0 -> 0; field.cuh:925-972).  Device pointers. */
panda_error panda_debug_field_op(unsigned field_id, unsigned op, void *d_r, const void *d_a, const void *d_b, size_t n, panda_stream stream);
/* op 0 = Jacobian + affine (madd), 1 = Jacobian + Jacobian, 2 = double, 3 / 4 = the four-lane spellings of 1 / 2 that the MSM's
 * fix-up and bucket-reduction trees run (csrc/curve29_quad.h); Jacobian in/out */
panda_error panda_debug_curve_op(unsigned curve, unsigned op, void *d_r, const void *d_a, const void *d_b, size_t n, panda_stream stream);
/* The field arithmetic on INTERNAL-form limbs, with no wire conversion, so that operands can sit anywhere inside the bounds contract of
 * csrc/fe29.h: an element is the N 29-bit limbs the kernels hold (in u32 words; 2 N for Fq2).  field id 0..5 as panda_debug_field_op,
 * 6 / 7 / 8 = Fq2 over BN254, BLS12-381, BLS12-377 Fq.  op: the table of csrc/fe29_debug_ops.h (0 = mul, 1 = sqr, 2 = mul_add, ...,
 * 14 = ext2_c0); inputs the op does not use may be NULL.  panda_error_invalid_value, with nothing launched, for a (field, op) pair
 * outside the table.  Device pointers. */
panda_error panda_debug_fe_internal(unsigned field_id, unsigned op, void *d_r, const void *d_a, const void *d_b, const void *d_c, const void *d_d, size_t n,
                                    panda_stream stream);
/* The XYZZ group law of csrc/curve29.h on INTERNAL-form points, with no wire conversion on the way in, so that a point can sit anywhere
 * inside the stored-point contract (X below (8+M) p loose, Y below YB p, ZZ and ZZZ below 2p tight).  A stored point is the 4 W u32
 * limbs the MSM kernels store (X, Y, ZZ, ZZZ; W = N limbs, 2 N for G2), an affine base 2 W limbs.  curve as panda_debug_curve_op;
 * op: the table of csrc/curve29_debug_ops.h (0 = madd_core, 1 = madd, 2 = madd_neg, 3 = madd_neg_raw, 4 = madd_trace, 5 = dbl_affine,
 * 6 = dbl, 7 = add, 8 / 9 = the four-lane add / dbl, 10..12 = to Jacobian wire, homogeneous wire, internal affine), which also gives
 * the width of r per element; d_a or d_b may be NULL where the op takes none.  panda_error_invalid_value, with nothing launched, for a
 * bad curve or a (curve, op) pair outside the table.  Device pointers. */
panda_error panda_debug_xyzz_internal(unsigned curve, unsigned op, void *d_r, const void *d_a, const void *d_b, size_t n, panda_stream stream);
/* Sets the scratch the entry points reuse between calls, so that a test can run a call on memory of its choosing: synchronises the
 * device, overwrites the WHOLE capacity of the calling thread's scratch arena on the current device and, if it has been allocated, the
 * calling thread's pinned mailbox, synchronises again, and reports the arena's base and capacity (either pointer may be NULL).
 *   mode 0: every byte becomes value & 0xFF.
 *   mode 1: 32-bit word i (i = 0, 1, ... from the base, taken modulo 2^32; the mailbox's words count from 0 again) becomes h(i ^ value),
 *           h(x): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16  in 32-bit arithmetic (a bijection).  The one
 *           to three bytes behind the arena's last whole word become value & 0xFF.
 * It allocates neither an arena nor a mailbox: with no arena it reports *base = NULL, *capacity = 0, and with neither it makes no
 * runtime call at all.  panda_error_invalid_value, with nothing written (*base and *capacity included), for any other mode.  What a
 * later call reserves beyond the capacity reported here is a fresh allocation, which this call did not fill. */
panda_error panda_debug_scratch_fill(unsigned mode, unsigned value, void **base, size_t *capacity);

const char *panda_version(void);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* PANDA_INTERFACE_H */
