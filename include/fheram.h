/*
 * fheram.h — C ABI of the MI355X-native FHE-RAM evaluator.
 *
 * Drop-in boundary for the hot path of phantomzone-org/fhe-ram (reference snapshot
 * 2026-02-13): Ram::read / Ram::read_prepare_write / Ram::write and the types either side of
 * them.  The reference has no FFI of its own (pure Rust over Poulpy); these entry points are
 * what a Rust `extern "C"` shim behind the crate's public API (src/lib.rs:12-21) binds — see
 * INTEGRATION.md for the binding.  Each entry cites the reference interface it replaces.
 *
 * Host data interchange = Poulpy's host layouts, little-endian int64:
 *   GLWE  (size limbs)                : [limb][col 2][N]
 *   GGSW  (dnum rows, size limbs)     : [row][col_in 2][limb][col_out 2][N]
 *   GGLWE key (dnum rows, size limbs) : [row][col_in 1][limb][col_out 2][N]
 * All uploaded limbs must be normalised: -2^(base2k-1) <= x < 2^(base2k-1).
 *
 * Threading contract = the reference's: every op takes `&mut self` (ram.rs:172,196,226), so
 * one op in flight per context; a context is not thread-safe.
 * Errors: the reference panics (assert!); this ABI returns a status and keeps a message.
 */
#ifndef FHERAM_H
#define FHERAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fheram_ctx fheram_ctx;   /* Ram<B> + Parameters<B> + EvaluationKeysPrepared (ram.rs:25-29) */
typedef struct fheram_addr fheram_addr; /* Address (address.rs:21-24), device resident              */

enum fheram_status {
    FHERAM_OK = 0,
    FHERAM_ERR_INVALID_ARG = 1,   /* size/layout asserts: ram.rs:144-155,243,404,482          */
    FHERAM_ERR_STATE = 2,         /* state-machine asserts: ram.rs:393-396,472-475,555-558   */
    FHERAM_ERR_UNINITIALIZED = 3, /* "unitialized memory": ram.rs:182-185,206-209            */
    FHERAM_ERR_KEYS = 4,          /* missing key / auto_key.p() != -1: coordinate_prepared.rs:134 */
    FHERAM_ERR_UNSUPPORTED = 5,   /* parameter set the kernels are not built for             */
    FHERAM_ERR_RANGE = 6,         /* a limb is not normalised                                */
    FHERAM_ERR_DEVICE = 7,        /* HIP runtime error                                       */
    FHERAM_ERR_PRECISION = 8      /* the FP64 round-off monitor saw |x - rint(x)| > 3/8 (no reference counterpart: Poulpy's FFT64
                                     backend, examples/fhe-ram.rs:3-7, rounds unchecked)     */
};

/* Parameters (parameters.rs:11-21,147-152). */
typedef struct fheram_params {
    uint32_t log_n;          /* LOG_N = 12                     parameters.rs:11 */
    uint32_t base2k;         /* BASE2K = 17                    parameters.rs:12 */
    uint32_t rank;           /* RANK = 1                       parameters.rs:13 */
    uint32_t k_glwe_pt;      /* K_GLWE_PT = 3                  parameters.rs:14 */
    uint32_t k_glwe_ct;      /* K_GLWE_CT = 3*BASE2K           parameters.rs:15 */
    uint32_t k_ggsw_addr;    /* K_GGSW_ADDR = 4*BASE2K         parameters.rs:16 */
    uint32_t k_evk_trace;    /* K_EVK_TRACE = 4*BASE2K         parameters.rs:17 */
    uint32_t k_evk_ggsw_inv; /* K_EVK_GGSW_INV = 5*BASE2K      parameters.rs:18 */
    uint32_t word_size;      /* WORDSIZE = 4                   parameters.rs:20 */
    uint32_t n_decomp;       /* len(DECOMP_N)                  parameters.rs:19 */
    uint8_t decomp_n[16];    /* DECOMP_N = [3,3,3,3]                            */
    uint64_t max_addr;       /* MAX_ADDR = 1<<14               parameters.rs:21 */
} fheram_params;

/* Parameters::new() defaults (parameters.rs:167-176). */
int fheram_params_default(fheram_params* out);

/* Ram::new / Ram::new_from_ram_params (ram.rs:59-87): allocates every device buffer the
 * context will ever need (rows, tree, packing scratch, prepared operands) on HIP device
 * `device`.  Mirrors Ram owning `subrams` + `scratch`. */
int fheram_ctx_create(const fheram_params* params, int device, fheram_ctx** out);
void fheram_ctx_destroy(fheram_ctx* ctx);
/* Message of the last failing call on ctx (ctx == NULL: last fheram_ctx_create failure). */
const char* fheram_last_error(const fheram_ctx* ctx);

/* Layout sizes in int64 elements (GLWELayout/GGSWLayout/GGLWELayout, parameters.rs:53-104). */
size_t fheram_glwe_len(const fheram_ctx* ctx);      /* glwe_ct_infos                    */
size_t fheram_ggsw_len(const fheram_ctx* ctx);      /* ggsw_infos                       */
size_t fheram_atk_len(const fheram_ctx* ctx);       /* evk_glwe_infos (one key)         */
size_t fheram_evk_inv_len(const fheram_ctx* ctx);   /* evk_ggsw_infos (one key)         */
size_t fheram_rows(const fheram_ctx* ctx);          /* GLWE rows per sub-RAM            */
int fheram_n_digits(const fheram_ctx* ctx);         /* GGSW digits of one Address       */
int fheram_n_coordinates(const fheram_ctx* ctx);    /* Address::n2 (address.rs:113)     */

/* EvaluationKeysPrepared::alloc + prepare (keys.rs:34-71): std-form keys in, device-prepared
 * (transform-domain) keys kept in the context.  gal_els must be GLWE::trace_galois_elements
 * (-1, 5^(2^(i-1)) mod 2N); atk_ggsw_inv_p must be -1 (coordinate_prepared.rs:134). */
int fheram_keys_load(fheram_ctx* ctx, const int64_t* gal_els, int n_gal, const int64_t* const* atk_glwe,
                     const int64_t* atk_ggsw_inv, int64_t atk_ggsw_inv_p, const int64_t* tsk_ggsw_inv);

/* Ram::encrypt_sk result hand-over (ram.rs:129-167): rows = [word_size][rows][GLWE]. The
 * encryption itself is the caller's (host) business.  Resets state to "readable". */
int fheram_ram_upload(fheram_ctx* ctx, const int64_t* rows);
int fheram_ram_download(fheram_ctx* ctx, int64_t* rows);
/* SubRam::tree level `level`, entry 0 of every sub-RAM: [word_size][GLWE] (ram.rs:300). */
int fheram_ram_tree_download(fheram_ctx* ctx, int level, int64_t* out);
/* SubRam::state (ram.rs:302): 1 after read_prepare_write, 0 after write. */
int fheram_ram_state(const fheram_ctx* ctx);

/* Address::alloc_from_params + encrypt_sk result hand-over (address.rs:58,86-109): n_ggsw
 * std-form GGSW digits, coordinate-major (coordinate 0 digits first). */
int fheram_address_create(fheram_ctx* ctx, const int64_t* const* ggsw, int n_ggsw, fheram_addr** out);
void fheram_address_destroy(fheram_addr* addr);

/* Ram::read (ram.rs:172-191).  out: [word_size][GLWE] int64, or NULL to leave the result on
 * the device (fetch it later with fheram_result_download). */
int fheram_read(fheram_ctx* ctx, const fheram_addr* addr, int64_t* out);
/* K = n_addr independent Ram::read (ram.rs:172-191) of the same RAM, as one operation.  A read does not change the RAM (only its
 * scratch), so the K reads share the rows, the keys and every address-independent launch; only the products with the address
 * digits are per address.
 * out (may be NULL): [n_addr][word_size][GLWE] int64; slice i is bit-identical to what fheram_read(ctx, addrs[i], ...) returns
 * on the same state.  Duplicates are allowed.  1 <= n_addr <= FHERAM_READ_BATCH_MAX.  Errors are those of fheram_read, checked
 * for every address before anything is enqueued; a row-sharded context is refused (FHERAM_ERR_INVALID_ARG).  Afterwards
 * fheram_result_download / _map return the result of addrs[n_addr-1], and the context is in the state the equivalent sequence
 * of reads leaves.  The batch's device buffers are allocated on first use and grown to the largest n_addr seen (FHERAM_ERR_DEVICE
 * if that fails; single reads still work); fheram_ctx_destroy frees them. */
#define FHERAM_READ_BATCH_MAX 8
int fheram_read_batch(fheram_ctx* ctx, const fheram_addr* const* addrs, int n_addr, int64_t* out);
/* Ram::read_prepare_write (ram.rs:196-222). */
int fheram_read_prepare_write(fheram_ctx* ctx, const fheram_addr* addr, int64_t* out);
/* Ram::write (ram.rs:226-294).  w: n_w GLWEs, each encrypting [w,0,...,0] (ram.rs:228);
 * w == NULL uses the words staged by fheram_word_stage. */
int fheram_write(fheram_ctx* ctx, const int64_t* w, int n_w, const fheram_addr* addr);
int fheram_word_stage(fheram_ctx* ctx, const int64_t* w, int n_w);
int fheram_result_download(fheram_ctx* ctx, int64_t* out);
/* The result of the last read / read_prepare_write in place: [word_size][GLWE] int64 in the context's pinned host buffer
 * (the device widens it straight into host memory; no copy on the host).  Valid until the next operation on ctx.  A Rust
 * shim builds its Vec<GLWE<Vec<u8>>> (ram.rs:176) from it with one copy instead of two. */
int fheram_result_map(fheram_ctx* ctx, const int64_t** out);
/* Block until every queued operation of ctx has finished. */
int fheram_sync(fheram_ctx* ctx);

/* ---- The exactness contract, checked.  The reference multiplies with Poulpy's FFT64 backend and rounds (examples/fhe-ram.rs:3-7);
 * so does csrc/fft_dev.hpp: the rounded output of an inverse transform is the exact integer only while the accumulated FP64
 * round-off stays below 1/2.  No a-priori bound below 1/2 is known for six accumulated terms of extreme limbs (measured worst
 * case found by search 0.25: DESIGN.md §2), so the roundings on the path report |x - rint(x)| to a per-context monitor
 * (fheram_config.monitor).  What it observes depends on the mode:
 *   monitor = 2 (what `safe` selects): every coefficient of every rounding.
 *   monitor = 1 (the default): a SAMPLE — one coefficient class per rounding site, class k = the coefficients j with j / 512 == k
 *     (a thread's k-th of eight), fixed at compile time (csrc/fft_dev.hpp):
 *         fft_inv_skew      first polynomial 0, second 3 (third 6)
 *         fft_inv1_hooked   5
 *         fft_inv2_hooked   first polynomial 1, second 4
 *     Classes 2 and 7 are observed nowhere, and a round-off confined to unobserved coefficients passes unseen.  Mode 1 detects the
 *     onset of a loss of precision that spreads over a polynomial (as accumulated FFT round-off does); it is not a guarantee for
 *     every coefficient (tests/test_gpu_fft_forms.py pins the table: a plant outside the sampled class returns FHERAM_OK).
 *   In both modes the observed quantity |x - rint(x)| cannot exceed 1/2: a true error e >= 1/2 reads as 1 - e (and the integer is
 *   already wrong), so the limit of 3/8 is a sound alarm only for errors below 5/8 — it catches round-off as it grows towards
 *   1/2, not an arbitrary corruption.
 *   After FHERAM_ERR_PRECISION from fheram_read_prepare_write or fheram_write (or the calls that wait for them) the RAM's rows
 *   are not to be trusted: the write has stored, or is storing, integers rounded from values the contract no longer covers.  Load
 *   the rows again; fheram_roundoff_reset only clears the flag.
 *   fheram_roundoff_max: waits for the context's streams; *max_out = the largest round-off seen since creation / the last reset;
 *                        returns FHERAM_ERR_PRECISION if it exceeds 3/8 — halfway between the largest round-off a search over
 *                        extreme operands has produced (1/4, tools/fft_search.hip) and failure (1/2); max_out is still written.
 *   Once a round-off above 3/8 was seen, every call that waits for the device (fheram_sync, the downloads of fheram_read /
 *   fheram_read_prepare_write / fheram_result_map / fheram_ram_download, fheram_timer_end) returns FHERAM_ERR_PRECISION until
 *   fheram_roundoff_reset.  No reference counterpart. */
int fheram_roundoff_max(fheram_ctx* ctx, double* max_out);
int fheram_roundoff_reset(fheram_ctx* ctx);

/* ---- Row-sharded RAM across the GPUs of a node.  The reference is single
 * threaded and has no counterpart; the split follows its control flow: the rows of one residue class
 * mod n_shards form a complete sub-tree of the GLWEPacker (bit-reversed feed, ram.rs:425-444), so a
 * shard that owns rows r = shard (mod n_shards) of every sub-RAM runs SubRam::read up to and
 * including its own packing levels; one exchange (all-gather of word_size GLWEs per shard) later the
 * root finishes the top log2(n_shards) levels, the coordinate-1 products and the trace.  Every
 * combine sees the same operands as in the sequential packer, so results are bit-identical.
 * Buffers are either host int64 ([..][GLWE], *_on_device = 0) or device int32 in the same
 * [limb][col][N] order (*_on_device = 1; the pointer must be valid on the context's device —
 * this is what an RCCL collective moves). */
int fheram_ctx_create_sharded(const fheram_params* params, int device, int shard, int n_shards, fheram_ctx** out);

/* Execution switches of a context: which decomposition the launchers of csrc/launch.hpp choose for a step and which launch form
 * (chain_form there) for a dependent chain.  Every setting
 * computes the same results (tests/test_gpu_parity.py and test_gpu_golden.py force each one); the defaults are the fastest
 * measured forms.  fheram_config_default() fills the library defaults and then applies the FHERAM_* environment overrides of
 * the same names (FHERAM_LIMB_SPLIT, _FINE_SPLIT, _MEMO, _PRE_INV, _TAIL, _TAIL_EP, _MID, _CHAIN, _CHAIN_Y, _PAIR_Z, _FUSE, _GRAPH,
 * _SAFE, _NCO, _MONITOR); fheram_ctx_create / _sharded use exactly that.  No reference counterpart (the reference has one code path). */
typedef struct fheram_config {
    int32_t limb_split;   /* 1: limb-parallel launches for batches far smaller than the chip */
    int32_t fine_split;   /* 1: one forward + one inverse transform per workgroup for <= 10 key-switches / <= 5 products */
    int32_t memo;         /* 1: Ram::write resumes from what read_prepare_write computed on the unchanged state */
    int32_t pre_inv;      /* 1: read_prepare_write starts the write's inverse digits behind a gate wave; 2: behind an event; 0: never */
    int32_t tail;         /* 1: the trace chain at the end of a read as one launch with in-kernel hand-offs (k_trace_tail) */
    int32_t tail_test;    /* test hook: 1 / 2 = every such launch gives up late (2 keeps the watch active) */
    int32_t mid;          /* 2: dependent chains on 9..64 ciphertexts as one launch (k_chain_mid); 1: the <= 16 split only; 0: off */
    int32_t mid_test;     /* test hook: one member of every such launch gives up */
    int32_t chain;        /* 1: a dependent chain of fused steps as one launch */
    int32_t chain_y;      /* 3: trace chains hand over through LDS and registers (ks_trace_l); 0: int32 limbs through global memory */
    int32_t pair_z;       /* 1: the column-split packer combine in closed form (k_pair_z) */
    int32_t fuse;         /* 1: a row's product chain and trace chain as one launch (k_read_chain / k_write_chain) */
    int32_t graph;        /* 1: replay each op's launch sequence from a hipGraph */
    int32_t safe;         /* 1: no in-kernel hand-offs between workgroups, no gate wave: stays inside the HIP memory model */
    int32_t nco;          /* output columns per workgroup: 1, 2, or 0 = chosen per launch */
    int32_t tail_ep;      /* 1 (default): coordinate 1's external products (>= 2 digits) run inside that launch, in front of the trace steps; 0: launches of their own */
    int32_t monitor;      /* round-off monitor (fheram_roundoff_max): 1 (default) every rounding of an inverse transform reports one of the thread's eight coefficients (which one differs between call sites); 2 all eight (what `safe` selects); 0 nothing is reported or checked */
    int32_t reserved;     /* must be 0 (a later version / size field): fheram_ctx_create_cfg refuses anything else */
} fheram_config;
/* ALWAYS start from fheram_config_default(): a zero-initialised struct is a valid configuration, but it selects every slow
 * path (no chains, no fused launches, no memo) and switches the round-off monitor off. */
void fheram_config_default(fheram_config* cfg);
/* fheram_ctx_create_sharded with explicit switches (cfg == NULL: fheram_config_default) */
int fheram_ctx_create_cfg(const fheram_params* p, int device, int shard, int n_shards, const fheram_config* cfg, fheram_ctx** out);
/* the switches IN EFFECT on this context (after `safe`, `graph` and `memo` have been applied to the others) */
int fheram_ctx_config(const fheram_ctx* ctx, fheram_config* out);

/* Stream ordering for DEVICE buffers (*_on_device = 1).  The evaluator enqueues on its own HIP stream;
 * a collective (RCCL) runs on the caller's.  Hand-overs of device buffers are asynchronous: no call
 * below blocks the host for them.  The caller orders the two streams with events instead:
 *   fheram_stream_signal(ctx, s): work enqueued on s AFTER this call waits for everything the context
 *                                 has enqueued so far (call it after fheram_read_partial / fheram_write_root,
 *                                 before the collective);
 *   fheram_stream_wait(ctx, s):   work the context enqueues AFTER this call waits for everything enqueued
 *                                 on s so far (call it after the collective, before fheram_read_finish /
 *                                 fheram_write_shard).
 * s is a hipStream_t (NULL = the legacy default stream).  Host buffers (*_on_device = 0) need neither. */
int fheram_stream_signal(fheram_ctx* ctx, void* hip_stream);
int fheram_stream_wait(fheram_ctx* ctx, void* hip_stream);
/* Exchange buffers on the context's device for a host that has no HIP binding of its own (hipMalloc /
 * hipFree): `bytes` of device memory, e.g. n_shards * word_size * fheram_glwe_len * 4 for the gathered
 * partials.  A host that already owns device memory (an RCCL / torch buffer) passes that instead. */
int fheram_device_malloc(fheram_ctx* ctx, size_t bytes, void** out);
int fheram_device_free(fheram_ctx* ctx, void* ptr);
int fheram_shard_info(const fheram_ctx* ctx, int* shard, int* n_shards, size_t* local_rows);
/* Every shard.  out: word_size partial GLWEs.  prepare_write != 0 keeps the rotated rows (ram.rs:502-504). */
int fheram_read_partial(fheram_ctx* ctx, const fheram_addr* addr, int prepare_write, void* out, int out_on_device);
/* Root.  partials: [n_shards][word_size] GLWEs in shard order.  out as in fheram_read (may be NULL). */
int fheram_read_finish(fheram_ctx* ctx, const fheram_addr* addr, int prepare_write, const void* partials,
                       int partials_on_device, int64_t* out);
/* Root: write_first_step + inverse coordinate-1 products (ram.rs:254-256,260-271,610).  ct_lo_out:
 * word_size GLWEs to broadcast. */
int fheram_write_root(fheram_ctx* ctx, const int64_t* w, int n_w, const fheram_addr* addr, void* ct_lo_out, int out_on_device);
/* Every shard, optional: start the part of a write that does not depend on ct_lo — trace(ct_hi) of the
 * local rows (ram.rs:616) and the inversion of coordinate 0 (ram.rs:278-289) — so that it runs while the
 * root computes ct_lo and the broadcast is in flight.  fheram_write_root and fheram_write_shard start
 * it themselves when it has not been started. */
int fheram_write_begin(fheram_ctx* ctx, const fheram_addr* addr);
/* Every shard: write_mid_step on its rows with the broadcast ct_lo, then write_last_step (ram.rs:612-630,644-648). */
int fheram_write_shard(fheram_ctx* ctx, const fheram_addr* addr, const void* ct_lo, int on_device);

/* ---- ONE RAM over the GPUs of a node behind ONE handle (reference API kept: one call per op,
 * ram.rs:172-176,196-200,226-231).  For a host that is a single process (a Rust `Ram` wrapper): the group owns one
 * row-shard context per device (rows r = shard (mod n) of every sub-RAM, as above), one host thread per device drives
 * it, and the two exchange steps — every shard's partial pack to the root for a read, the root's ct_lo to every shard
 * for a write — are peer-to-peer device copies (xGMI) ordered by events: no host staging, no collective library.
 * fhe-ram_amd/sharded.py drives the per-shard entry points above from one PROCESS per GPU over RCCL instead; both give
 * the results of the unsharded path bit for bit.  n_devices must be a power of two <= rows per sub-RAM (1 = plain
 * context); the same device may be named several times (rehearsal on one GPU).  Group ops are synchronous: they return
 * when the op is complete on every shard.  One op in flight per group (the reference's `&mut self`). */
typedef struct fheram_group fheram_group;
typedef struct fheram_group_addr fheram_group_addr;
int fheram_group_create(const fheram_params* params, const int* devices, int n_devices, fheram_group** out);   /* Ram::new, ram.rs:59-87 */
void fheram_group_destroy(fheram_group* grp);
const char* fheram_group_last_error(const fheram_group* grp);   /* grp == NULL: last fheram_group_create failure */
int fheram_group_size(const fheram_group* grp);
/* the shard context behind the group (setup-side calls per shard: fheram_ram_encrypt_sk, fheram_keys_encrypt_sk, ...);
 * not to be used while a group op is in flight */
fheram_ctx* fheram_group_ctx(fheram_group* grp, int shard);
int fheram_group_keys_load(fheram_group* grp, const int64_t* gal_els, int n_gal, const int64_t* const* atk_glwe,
                           const int64_t* atk_ggsw_inv, int64_t atk_ggsw_inv_p, const int64_t* tsk_ggsw_inv);   /* keys.rs:57-71, replicated */
/* rows: the WHOLE RAM [word_size][rows][GLWE] (Ram::encrypt_sk output, ram.rs:129-167); scattered / gathered by shard */
int fheram_group_ram_upload(fheram_group* grp, const int64_t* rows);
int fheram_group_ram_download(fheram_group* grp, int64_t* rows);
int fheram_group_ram_tree_download(fheram_group* grp, int level, int64_t* out);
int fheram_group_ram_state(const fheram_group* grp);
int fheram_group_address_create(fheram_group* grp, const int64_t* const* ggsw, int n_ggsw, fheram_group_addr** out);   /* address.rs:58,86-109, replicated */
void fheram_group_address_destroy(fheram_group_addr* addr);
int fheram_group_read(fheram_group* grp, const fheram_group_addr* addr, int64_t* out);                 /* Ram::read, ram.rs:172-191 */
int fheram_group_read_prepare_write(fheram_group* grp, const fheram_group_addr* addr, int64_t* out);   /* ram.rs:196-222 */
int fheram_group_write(fheram_group* grp, const int64_t* w, int n_w, const fheram_group_addr* addr);   /* ram.rs:226-294; w == NULL: staged words */
int fheram_group_word_stage(fheram_group* grp, const int64_t* w, int n_w);
int fheram_group_result_download(fheram_group* grp, int64_t* out);
/* Exchange path of the group (round 4).  fheram_group_create runs one self-test copy per shard in both directions (shard -> root as a
 * read's partial pack, root -> shard as a write's ct_lo) and fails with FHERAM_ERR_DEVICE, naming the pair, if the bytes do not arrive.
 * direct[i] = 1: the runtime reports a peer-to-peer path between shard i's device and the root's (or they are one device); 0: staged. */
int fheram_group_peer_info(const fheram_group* grp, int* direct, int n);
/* 1 after a group op failed part-way (work had been enqueued on some shard): rows and state flags of the shards are inconsistent,
 * every further op returns FHERAM_ERR_STATE until fheram_group_ram_upload has replaced the rows.  Calls the reference would refuse
 * with an assert (wrong state, foreign address, ram.rs:393-396,404,472-475,555-558) are refused before anything is enqueued and
 * poison nothing. */
int fheram_group_poisoned(const fheram_group* grp);
/* the largest round-off over the shards' monitors (fheram_roundoff_max on every shard) */
int fheram_group_roundoff_max(fheram_group* grp, double* max_out);

/* ---- bank: M RAMs of the same shape under ONE prepared key set on one GPU, and Ram::read / read_prepare_write / write on a
 * contiguous range of them as ONE operation, one address per member.  Ram objects are independent units (ram.rs:25-29; `&mut self`
 * serialises operations per RAM only): nothing orders operations on different RAMs, so their latency-bound steps (pair levels,
 * coordinate-1 products, traces, the write's head) run as single launches over n * word_size ciphertexts, and the rows' chains as one
 * launch with a per-member operand table.
 * Semantics: a bank of M members behaves exactly like M contexts created with the same fheram_params / fheram_config, loaded with
 * the same keys and rows and given the same per-member sequence of operations: every result, every row after a write, tree level 0
 * and the state flag of member m are int64-identical to those of standalone context m.
 * An operation names members [first, first + n) and n addresses (created with fheram_bank_address_create; the same handle may serve
 * several members); members outside the range are untouched.  A range of one member is the plain operation on that member, so a host
 * mixes operations by issuing ranges (a read on member 0 while member 1 sits between read_prepare_write and write).
 * Every check — the state machine per member (ram.rs:393-396,472-475,555-558), uninitialised rows, missing keys, foreign addresses,
 * null arguments — runs for the whole range before anything is enqueued: a refused call changes no member.
 * A bank is never row-sharded and never part of a group.  One op in flight per bank; a bank is not thread-safe. */
#define FHERAM_BANK_MAX 8
typedef struct fheram_bank fheram_bank;
/* cfg == NULL: fheram_config_default().  Checks, in this order: null pointers, n_members outside [1, FHERAM_BANK_MAX] and
 * n_members * word_size > 64 (FHERAM_ERR_INVALID_ARG); the parameter checks of fheram_ctx_create_cfg (same codes and messages);
 * only then "no HIP device" (FHERAM_ERR_DEVICE).  In a bank of more than one member the write's inverse digits are never started
 * early (pre_inv reads as 0); a bank of one member is a plain context. */
int fheram_bank_create(const fheram_params* params, int device, int n_members, const fheram_config* cfg, fheram_bank** out);
void fheram_bank_destroy(fheram_bank* bank);
const char* fheram_bank_last_error(const fheram_bank* bank);   /* bank == NULL: last fheram_bank_create failure */
int fheram_bank_size(const fheram_bank* bank);
/* ONE prepared key set for all members (keys.rs:57-71); arguments as fheram_keys_load */
int fheram_bank_keys_load(fheram_bank* bank, const int64_t* gal_els, int n_gal, const int64_t* const* atk_glwe,
                          const int64_t* atk_ggsw_inv, int64_t atk_ggsw_inv_p, const int64_t* tsk_ggsw_inv);
int fheram_bank_ram_upload(fheram_bank* bank, int member, const int64_t* rows);   /* [word_size][rows][GLWE]; the member becomes readable */
int fheram_bank_ram_download(fheram_bank* bank, int member, int64_t* rows);
int fheram_bank_ram_tree_download(fheram_bank* bank, int member, int level, int64_t* out);
int fheram_bank_ram_state(const fheram_bank* bank, int member);
/* an Address bound to the bank (any member); freed with fheram_address_destroy */
int fheram_bank_address_create(fheram_bank* bank, const int64_t* const* ggsw, int n_ggsw, fheram_addr** out);
/* out: [n][word_size][GLWE], or NULL (no download: fheram_bank_result_download later) */
int fheram_bank_read(fheram_bank* bank, int first, int n, const fheram_addr* const* addrs, int64_t* out);
int fheram_bank_read_prepare_write(fheram_bank* bank, int first, int n, const fheram_addr* const* addrs, int64_t* out);
/* w: [n][word_size][GLWE], member first + k's words at k */
int fheram_bank_write(fheram_bank* bank, int first, int n, const int64_t* w, const fheram_addr* const* addrs);
/* the results of each member's last read / read_prepare_write */
int fheram_bank_result_download(fheram_bank* bank, int first, int n, int64_t* out);
/* A read list: reads of ANY members as one operation — any order, any repetition, any subset (a VM step that reads rs1 and rs2 from
 * the register file, an instruction word and a data word: members {0, 0, 1, 2}).  The latency-bound end of a read is paid once for the
 * list, and the rows' chains of all entries are one launch.  Slice k of the results is int64-identical to what
 * fheram_bank_read(bank, members[k], 1, &addrs[k], ...) returns on the same state, and the bank is afterwards where the sequence of
 * those n single-member reads leaves it: every named member in state 0 with rows and tree level 0 unchanged,
 * fheram_bank_result_download of it returning the result of the LAST entry that named it; members that are not named are untouched in
 * every respect (one that sits between read_prepare_write and write resumes its write from what it kept: the list runs on buffers of
 * its own, allocated on first use, grown to the largest list seen and freed with the bank).
 * 1 <= n <= FHERAM_READ_LIST_MAX and n * word_size <= 64.  Checked for the whole list before anything is enqueued, a refused call
 * changes nothing: null pointers, n out of range, a member index outside the bank, a foreign or empty address
 * (FHERAM_ERR_INVALID_ARG); a named member without rows (FHERAM_ERR_UNINITIALIZED); keys not loaded (FHERAM_ERR_KEYS); a named member
 * between read_prepare_write and write (FHERAM_ERR_STATE).  FHERAM_ERR_DEVICE: the list's buffers cannot be allocated (every other
 * operation still works).  The write side's list form is fheram_bank_read_prepare_write_list / fheram_bank_write_list below. */
#define FHERAM_READ_LIST_MAX 8
/* K = n independent Ram::read (ram.rs:172-191), entry k on member members[k] at addrs[k], as ONE operation.
 * Any order, any repetition, any subset of the bank's members.  out: [n][word_size][GLWE], or NULL (no host wait). */
int fheram_bank_read_list(fheram_bank* bank, const int* members, const fheram_addr* const* addrs, int n, int64_t* out);
/* entries [first, first + n) of the LAST list, [n][word_size][GLWE]; for a list that was enqueued with out == NULL.
 * FHERAM_ERR_STATE before any list has run, FHERAM_ERR_INVALID_ARG for a slice outside the last list. */
int fheram_bank_read_list_result(fheram_bank* bank, int first, int n, int64_t* out);
/* A write list: read_prepare_write / write on ANY set of members as one operation — distinct members, any order, any subset (members
 * {0, 2} of a bank of three: a register file and a data memory with a ROM between them), 1 <= n <= fheram_bank_size(bank); a RAM has
 * one pending write (ram.rs:196-294), so no member is named twice.  The latency-bound ends of both halves are paid once for the list,
 * and the rows' chains of all entries are one launch each, on the members' own rows.  The call is int64-identical to the n
 * single-member calls fheram_bank_read_prepare_write(bank, members[k], 1, &addrs[k], ..) / fheram_bank_write(bank, members[k], 1, ..):
 * slice k of out is member members[k]'s result, and afterwards every named member has the state flag, rows, tree level 0 and
 * fheram_bank_result_download result of a standalone context driven the same way.  A write list may name any members in state 1,
 * however they were prepared (a list, a range, a single call), and members prepared by a list may be written by ranges or single
 * calls; what a write resumes from is an optimisation that never changes a result.  Members that are not named are untouched in every
 * respect: one between read_prepare_write and write keeps what it kept, the results of the last read list stay readable, and a read
 * list on other members may run between the two halves (the write lists run on buffers of their own, allocated on first use, grown
 * to the largest list seen and freed with the bank).  A list of one entry is the plain single-member operation, a contiguous
 * ascending run the range operation.  Neither call waits for the device (out == NULL for the first).
 * Checked for the whole list before anything is enqueued, a refused call changes nothing: null pointers, n out of range, a member
 * index outside the bank, a member named twice, a foreign or empty address (FHERAM_ERR_INVALID_ARG); a named member without rows
 * (FHERAM_ERR_UNINITIALIZED); keys not loaded (FHERAM_ERR_KEYS); read_prepare_write naming a member in state 1, write naming a member
 * in state 0 (FHERAM_ERR_STATE); a word limb out of range (FHERAM_ERR_RANGE, as fheram_bank_write: no row is touched and the members
 * stay prepared).  FHERAM_ERR_DEVICE: the lists' buffers cannot be allocated (every other operation still works). */
/* entry k: Ram::read_prepare_write (ram.rs:196-222) of member members[k] at addrs[k]; out: [n][word_size][GLWE] or NULL (no host wait) */
int fheram_bank_read_prepare_write_list(fheram_bank* bank, const int* members, const fheram_addr* const* addrs, int n, int64_t* out);
/* entry k: Ram::write (ram.rs:226-294) of w[k] ([n][word_size][GLWE]) to member members[k] at addrs[k] */
int fheram_bank_write_list(fheram_bank* bank, const int* members, const fheram_addr* const* addrs, int n, const int64_t* w);
/* Self-test of the FHERAM_ERR_DEVICE path of the two calls above (not on the RAM path): the nth device allocation their buffers ask for
 * from now on fails once, as an exhausted device would make it (nth = 1: the next one; 0: none, which withdraws an earlier request).
 * The buffers are eleven allocations, made when a list is longer than any before it. */
int fheram_bank_selftest_fail_list_alloc(fheram_bank* bank, int nth);
int fheram_bank_sync(fheram_bank* bank);
/* one round-off monitor for the bank; FHERAM_ERR_PRECISION as for a context */
int fheram_bank_roundoff_max(fheram_bank* bank, double* max_out);
int fheram_bank_roundoff_reset(fheram_bank* bank);
/* as fheram_tail_stats / fheram_mid_stats / fheram_profile_*: the launch classes are those of a context */
int fheram_bank_tail_stats(fheram_bank* bank, uint64_t* launches, uint64_t* fallbacks);
int fheram_bank_mid_stats(fheram_bank* bank, uint64_t* launches, uint64_t* fallbacks);
int fheram_bank_profile_enable(fheram_bank* bank, int on);
int fheram_bank_profile_get(fheram_bank* bank, const char* kernel_class, uint64_t* launches, uint64_t* blocks, double* total_ms);
int fheram_bank_profile_reset(fheram_bank* bank);

/* ---- Poulpy-level operations reached from the path, exposed for
 * parity tests and micro-benchmarks.  Inputs/outputs are host buffers in the layouts above. */

/* glwe_external_product (coordinate_prepared.rs:156): res[i] = a[i] (x) ggsw, i < batch. */
int fheram_glwe_external_product(fheram_ctx* ctx, const int64_t* a, int batch, const int64_t* ggsw, int64_t* res);
/* glwe_automorphism family with the loaded trace key of Galois element gal_el:
 * mode 0: res = phi(KS(a));  1: res = a + phi(KS(a));  2: res = a - phi(KS(a)). */
int fheram_glwe_automorphism(fheram_ctx* ctx, int mode, int64_t gal_el, const int64_t* a, int batch, int64_t* res);
/* GLWE::trace(start, end) (ram.rs:457,540,572,616,621). */
int fheram_glwe_trace(fheram_ctx* ctx, int start, int end, const int64_t* a, int batch, int64_t* res);
/* GLWEPacker (ram.rs:425-448): packs coefficient 0 of cts[0..count) into coefficients
 * 0..count of one GLWE, feeding them in the RAM's bit-reversed order. */
int fheram_glwe_pack(fheram_ctx* ctx, const int64_t* cts, int count, int64_t* out);
/* GGSW::automorphism(p=-1) + tensor-key row expansion (coordinate_prepared.rs:138). */
int fheram_ggsw_automorphism_inv(fheram_ctx* ctx, const int64_t* ggsw_in, int64_t* ggsw_out);

/* ---- Setup side on the device: secret-key encryption of the RAM, of
 * addresses and of the evaluation keys, and decryption.  SAMPLING STAYS ON THE HOST: the caller
 * draws the uniform mask limbs and the rounded-Gaussian noise polynomials from its own sources
 * (Poulpy's `Source` in a Rust host: source_xa / source_xe of the calls cited below) and hands them
 * over; the device does the arithmetic (products with the secret, limb normalisation, key
 * preparation).  The same draws therefore give the same ciphertexts as the host implementation.
 * Per GLWE of `size` limbs, in the order the reference encrypts them: mask = size*N limbs in
 * [-2^16, 2^16) (limb-major), noise = N integers already scaled to the ciphertext precision k
 * (added on limb ceil(k/base2k)-1; |e| < 2^30). */
typedef struct fheram_secret fheram_secret;
/* GLWESecret + GLWESecretPrepared (examples/fhe-ram.rs:49-59): sk = N coefficients in {-1,0,1}. */
int fheram_secret_create(fheram_ctx* ctx, const int64_t* sk, fheram_secret** out);
void fheram_secret_destroy(fheram_secret* sk);
/* GLWE::encrypt_sk (Poulpy; call sites ram.rs:369-376, examples/fhe-ram.rs:179-210) on n_glwe
 * ciphertexts of `size` limbs (3, 4 or 5) at precision k.  pt: [n_glwe][pt_size][N] normalised
 * limbs or NULL (encryption of zero); pt_col 0 adds it to the body, 1 to the mask column after
 * the product with the secret (GGSW rows).  out: [n_glwe][size][2][N]. */
int fheram_glwe_encrypt_sk(fheram_ctx* ctx, const fheram_secret* sk, int n_glwe, int size, int k, const int64_t* pt,
                           int pt_size, int pt_col, const int64_t* mask, const int64_t* noise, int64_t* out);
/* GLWE::decrypt (examples/fhe-ram.rs:217-222): pt[i] = normalise(body + mask*s), [n_glwe][size][N]. */
int fheram_glwe_decrypt(fheram_ctx* ctx, const fheram_secret* sk, int n_glwe, int size, const int64_t* ct, int64_t* pt);
/* Ram::encrypt_sk (ram.rs:129-167, SubRam::encrypt_sk ram.rs:334-380): data = max_addr*word_size
 * bytes, interleaved by word as in the reference.  mask [word_size][rows][3][N], noise
 * [word_size][rows][N] for the rows THIS context holds (all of them unless sharded; a shard owns
 * global rows shard + x*n_shards).  The rows are encrypted straight into device memory. */
int fheram_ram_encrypt_sk(fheram_ctx* ctx, const fheram_secret* sk, const uint8_t* data, size_t data_len,
                          const int64_t* mask, const int64_t* noise);
/* Address::encrypt_sk (address.rs:86-109) -> Coordinate::encrypt_sk (coordinate.rs:121-180): GGSW
 * digits of -value per coordinate.  mask [n_digits][3 rows][2 col_in][4][N], noise
 * [n_digits][3][2][N], digits coordinate-major.  The address is created on the device. */
int fheram_address_encrypt_sk(fheram_ctx* ctx, const fheram_secret* sk, uint32_t value, const int64_t* mask,
                              const int64_t* noise, fheram_addr** out);
/* The std-form GGSW digits of an address, [n_digits][fheram_ggsw_len] (parity tests, hand-over to a host). */
int fheram_address_download(fheram_ctx* ctx, const fheram_addr* addr, int64_t* out);
/* EvaluationKeys::encrypt_sk (keys.rs:135-180) + EvaluationKeysPrepared::prepare (keys.rs:57-71):
 * the log2(N) trace keys in GLWE::trace_galois_elements order (3 rows of 4 limbs each), then the
 * tensor key, then the p = -1 key (4 rows of 5 limbs each): mask = (36*4 + 8*5)*N limbs, noise =
 * 44*N.  Keys are generated and prepared on the device; std_out (optional, may be NULL) receives
 * the std forms [12][fheram_atk_len] ++ tensor [fheram_evk_inv_len] ++ inverse [fheram_evk_inv_len]. */
int fheram_keys_encrypt_sk(fheram_ctx* ctx, const fheram_secret* sk, const int64_t* mask, const int64_t* noise,
                           int64_t* std_out);

/* ---- Address::set_from_fheuint (conversion.rs:18-82).
 * *** CONTRACT-COMPATIBLE ONLY — THE INPUT LAYOUT IS NOT poulpy-schemes' ***  A Rust host cannot hand its own FheUintPrepared
 * to fheram_fheuint_create: poulpy-schemes 0.3.3 is un-vendored (Cargo.toml:10), so neither the memory layout of
 * FheUintPrepared nor the algorithm of scalar_to_ggsw_blind_rotation could be read; the type below is this library's own.  What
 * these entry points guarantee is the reference test's contract (conversion.rs:100-220): digit d decrypts to
 * X^{((k >> bit_rsh) mod 2^bit_mask) << bit_lsh} on the gadget within the test's noise bound.  tools/poulpy_kat (feature
 * kat_fheuint) exports a real FheUintPrepared and one derived digit for the first Rust-equipped run to compare against.
 * The reference derives every address
 * digit from an encrypted integer with poulpy-schemes' scalar_to_ggsw_blind_rotation (un-vendored); what is built
 * here is its CONTRACT (conversion.rs:41-65 and the test at :100-220), by CMux chains on noiseless GGSW rows with
 * the external-product kernels — a self-consistent restatement, bit-exact against the in-repo oracle only.
 * FheUintPrepared<u32> = one GGSW per bit, LSB first, in the layout of the GGSW-inversion keys
 * (k = k_evk_ggsw_inv, 5 limbs, dnum 4): [n_bits][row 4][col_in 2][limb 5][col_out 2][N] int64. */
typedef struct fheram_fheuint fheram_fheuint;
size_t fheram_fheuint_ggsw_len(const fheram_ctx* ctx);
/* FheUintPrepared::alloc + prepare from host ciphertexts. */
int fheram_fheuint_create(fheram_ctx* ctx, const int64_t* bits, int n_bits, fheram_fheuint** out);
/* FheUintPrepared::encrypt_sk (conversion.rs:160-168) on the device with host-drawn randomness (as the other
 * encrypt_sk entry points): mask [n_bits][4][2][5][N], noise [n_bits][4][2][N]. */
int fheram_fheuint_encrypt_sk(fheram_ctx* ctx, const fheram_secret* sk, uint32_t value, int n_bits, const int64_t* mask,
                              const int64_t* noise, fheram_fheuint** out);
int fheram_fheuint_download(fheram_ctx* ctx, const fheram_fheuint* fu, int64_t* out);
void fheram_fheuint_destroy(fheram_fheuint* fu);
/* Address::set_from_fheuint (conversion.rs:68-82): digit d = GGSW of X^{+-(((k >> bit_rsh) mod 2^bit_mask) << bit_lsh)}
 * over the context's digit plan; sign != 0: + (what the reference's test decrypts to), 0: - (the convention of
 * Address::encrypt_sk, address.rs:102-108, i.e. an address Ram::read accepts). */
int fheram_address_set_from_fheuint(fheram_ctx* ctx, const fheram_fheuint* fu, int sign, fheram_addr** out);

/* ---- The same conversion on a step's critical path: K addresses from K encrypted integers as ONE launch, into existing addresses.
 * (The CONTRACT-COMPATIBLE-ONLY warning above applies unchanged: same input type, same contract, same digits bit for bit.) */
#define FHERAM_DERIVE_MAX 8
/* an address with its device buffers and no digits yet; read / write refuse it (FHERAM_ERR_INVALID_ARG, "empty address") until derived */
int fheram_address_alloc(fheram_ctx* ctx, fheram_addr** out);
/* addrs[i] <- Address::set_from_fheuint(fus[i]) for i < n, as ONE launch enqueued on the context's stream.  No allocation, no
 * host wait: returns once enqueued; later operations of ctx that use addrs[i] are ordered behind it.  sign as in
 * fheram_address_set_from_fheuint.  addrs[i] may come from fheram_address_alloc, _create, _encrypt_sk or an earlier derivation
 * (overwritten in place).  The integers must stay alive until the context has been synchronised.
 * Every check runs for the whole list before anything is enqueued (a refused call changes no address); FHERAM_ERR_INVALID_ARG:
 * null pointers, n outside [1, FHERAM_DERIVE_MAX], an integer or address of another context or bank, an integer narrower than
 * the address plan, the same address twice in addrs (the same integer twice in fus is allowed).  FHERAM_ERR_UNSUPPORTED: a digit
 * plan of more than 8 digits (use fheram_address_set_from_fheuint). */
int fheram_address_derive(fheram_ctx* ctx, const fheram_fheuint* const* fus, int n, int sign, fheram_addr* const* addrs);
/* The same on a bank: integers and addresses bound to the bank (any member).  A derived address is an ordinary bank address
 * (fheram_bank_address_create's kind) and may serve several members.  Integers are freed with fheram_fheuint_destroy, addresses
 * with fheram_address_destroy. */
int fheram_bank_fheuint_create(fheram_bank* bank, const int64_t* bits, int n_bits, fheram_fheuint** out);
int fheram_bank_address_alloc(fheram_bank* bank, fheram_addr** out);
int fheram_bank_address_derive(fheram_bank* bank, const fheram_fheuint* const* fus, int n, int sign, fheram_addr* const* addrs);
/* Addresses from a BIT OFFSET of the integers: addrs[k] <- the address whose plan reads bits [first_bit[k], first_bit[k] + plan bits) of
 * fus[k] — fheram_address_derive with the plan's bit_rsh advanced by first_bit[k] (a byte-addressed load or store takes its word
 * address from bits [2, ..) and its lane offset from bits [0, 2) of the same integer).  One launch per DISTINCT first_bit; the checks,
 * the stream ordering and the fresh address ids are fheram_address_derive's (one body), and with first_bit all zero the digits are
 * fheram_address_derive's bit for bit.  Also FHERAM_ERR_INVALID_ARG: first_bit null, first_bit[k] < 0, first_bit[k] + plan bits beyond
 * the integer's width. */
int fheram_address_derive_at(fheram_ctx* ctx, const fheram_fheuint* const* fus, const int* first_bit, int n, int sign, fheram_addr* const* addrs);
int fheram_bank_address_derive_at(fheram_bank* bank, const fheram_fheuint* const* fus, const int* first_bit, int n, int sign, fheram_addr* const* addrs);

/* ---- Oblivious select on a bank: pick one of m candidate words by an ENCRYPTED index, on the device — a VM step's write enable
 * (`enable ? new : old`), its store merge and result pick, and its moves between memories, without a host round trip.
 * *** CONTRACT-COMPATIBLE ONLY *** (as fheram_address_derive above): what is restated is the selection step that the reference's
 * select_store (store.rs:40-67) and select_rd (arithmetic.rs:212-231) share — "blind-rotate a packed ciphertext by an encrypted index,
 * then trace" — in this library's own arithmetic, where it is exactly Ram::read (ram.rs:451,457) on a ONE-ROW RAM of max_addr = 2^bits
 * whose row packs candidate j at coefficient j and whose address is the index.  Their callers (the BDD circuits, splice_u8 / splice_u16)
 * are un-vendored and out of scope.
 * A SELECTOR of `bits` bits is the Address of such a RAM: the digit plan get_base_2d(2^bits) gives over the bank's DECOMP_N (one
 * coordinate; [3,3,3,3] gives [1] [2] [3] [3,1] [3,2] for bits = 1..5), each digit the GGSW of X^-v (the sign of Address::encrypt_sk,
 * sign = 0 of fheram_address_derive) in the layout of address digits (k_ggsw_addr: 4 limbs, dnum 3). */
#define FHERAM_SELECT_BITS_MAX 5          /* up to 32 candidates */
#define FHERAM_SELECT_MAX 8               /* selects per call; n * word_size <= 64 as for the lists */
#define FHERAM_SELECTOR_WIDE_DIGITS_MAX 5 /* digits of a WIDE selector (the address of a table, below): what a selector's plan holds */
typedef struct fheram_selector fheram_selector;
/* buffers and no digits: fheram_bank_select refuses it (FHERAM_ERR_INVALID_ARG) until it has been derived */
int fheram_bank_selector_alloc(fheram_bank* bank, int bits, fheram_selector** out);
/* from n_ggsw host std-form digits (n_ggsw must be the plan's digit count: fheram_selector_n_digits) */
int fheram_bank_selector_create(fheram_bank* bank, const int64_t* const* ggsw, int n_ggsw, int bits, fheram_selector** out);
/* sels[i] <- bits [first_bit[i], first_bit[i] + bits_i) of fus[i], in place (a selector from _alloc, _create or an earlier derivation),
 * through k_cmux_chain: one launch per distinct (first_bit, bits) pair, no allocation, no host wait; later selects are ordered behind it
 * on the bank's stream.  The integers must stay alive until the bank has been synchronised.  Checked for the whole list before anything
 * is enqueued, a refused call changes nothing (FHERAM_ERR_INVALID_ARG): null pointers, n outside [1, FHERAM_SELECT_MAX], a selector or
 * integer of another bank, first_bit + bits beyond the integer's width, the same selector twice. */
int fheram_bank_selector_derive(fheram_bank* bank, const fheram_fheuint* const* fus, const int* first_bit, int n, fheram_selector* const* sels);
/* the std-form digits, [n_digits][fheram_ggsw_len] */
int fheram_bank_selector_download(fheram_bank* bank, const fheram_selector* sel, int64_t* out);
int fheram_selector_n_digits(const fheram_selector* sel);
void fheram_selector_destroy(fheram_selector* sel);
/* Where a candidate word (word_size GLWEs, each encrypting [v, 0, .., 0]) comes from. */
enum { FHERAM_SRC_ZERO = 0,            /* all-zero ciphertexts                                                                */
       FHERAM_SRC_HOST = 1,            /* slot `index` of host_words ([..][word_size][GLWE]), range-checked as write words are */
       FHERAM_SRC_MEMBER_RESULT = 2,   /* member `index`'s last read / read_prepare_write result                              */
       FHERAM_SRC_LIST_RESULT = 3,     /* entry `index` of the last read list                                                 */
       FHERAM_SRC_SELECT_RESULT = 4 }; /* output `index` of the previous select call                                          */
/* two more kinds, of a bank's register files (below); valid wherever a fheram_select_src or a fheram_select_lane is taken */
#define FHERAM_SRC_REGS_RESULT 5       /* output `index` of the bank's last fheram_bank_regs_read                              */
#define FHERAM_SRC_REGS_OLD 6          /* the bank's last fheram_bank_regs_read_prepare_write result; index must be 0          */
/* one more, of a bank's tables (below); valid in the same places.  (Kind 7 is unknown.) */
#define FHERAM_SRC_TABLE_RESULT 8      /* output `index` of the bank's last fheram_bank_table_read                             */
typedef struct fheram_select_src { int32_t kind, index; } fheram_select_src;
/* n selects as ONE operation.  Select k has the candidates srcs[off_k .. off_k + n_cand[k]), off_k = the sum of the earlier n_cand, and
 * for every word ciphertext y
 *     packed_y = glwe_normalize( sum_{j < n_cand[k]} X^j * c_j[y] )          (one launch for the whole call: k_select_pack)
 *     out_k[y] = Ram::read of the one-row RAM {packed_y} (max_addr = 2^bits) at sels[k]: the products with its digits in order, then
 *                trace(0, log N) — the launches a read's top enqueues, in the forms the bank's configuration selects.
 * The selected index i < n_cand[k] gives candidate i; an index >= n_cand[k] an encryption of 0.  All selectors of one call have the
 * same `bits` (one digit count for the operand table).  out: [n][word_size][GLWE], or NULL (no host wait; fheram_bank_select_result later).
 * The select runs on buffers of its own (allocated on first use, grown to the largest call, freed with the bank; FHERAM_ERR_DEVICE if
 * that fails, every other operation still works): no member's rows, state flag, tree, result or kept memo changes — a member between
 * read_prepare_write and write resumes its write exactly as before — and the last read list's results stay readable.
 * Checked before anything is enqueued, a refused call changes nothing.  FHERAM_ERR_INVALID_ARG: null arguments, n outside
 * [1, FHERAM_SELECT_MAX], n * word_size > 64, n_cand[k] outside [1, 2^bits], a foreign or underived selector, selectors of different
 * bits, an unknown source kind, an index outside the bank, the last list or the last select, a HOST source with host_words == NULL;
 * FHERAM_ERR_KEYS: keys not loaded; FHERAM_ERR_STATE: a MEMBER_RESULT member without a result, a LIST_RESULT / SELECT_RESULT source
 * when no such operation has run; FHERAM_ERR_RANGE: a host limb out of range. */
int fheram_bank_select(fheram_bank* bank, const fheram_selector* const* sels, const int* n_cand, int n,
                       const fheram_select_src* srcs, const int64_t* host_words, int64_t* out /* [n][word_size][GLWE] or NULL */);
/* outputs [first, first + n) of the LAST select; FHERAM_ERR_STATE before any select has run */
int fheram_bank_select_result(fheram_bank* bank, int first, int n, int64_t* out);
/* entry k: Ram::write (ram.rs:226-294) of output picks[k] of the last fheram_bank_select to member members[k] at addrs[k].  Checks and
 * semantics are those of fheram_bank_write_list; the words are copied on the device (no host wait, no range check: a select's outputs
 * are normalised by construction), and rows and results are int64-identical to fheram_bank_write_list given the downloaded outputs.
 * Also FHERAM_ERR_STATE: no select has run; FHERAM_ERR_INVALID_ARG: a pick outside the last select. */
int fheram_bank_write_list_selected(fheram_bank* bank, const int* members, const fheram_addr* const* addrs, int n, const int* picks);
/* Self-test of fheram_bank_select's FHERAM_ERR_DEVICE path, as fheram_bank_selftest_fail_list_alloc: the nth device allocation its
 * buffers ask for from now on fails once (0 withdraws the request). */
int fheram_bank_selftest_fail_select_alloc(fheram_bank* bank, int nth);

/* ---- Sub-word loads and stores: select candidates assembled LANE BY LANE, and selectors made of fields of different integers.
 * *** CONTRACT-COMPATIBLE ONLY *** as the select above: the same selection step (Ram::read on a one-row RAM) with candidates put
 * together from whole byte ciphertexts.  A word is word_size GLWEs, one per byte (sub-RAM w holds byte w of every word, ram.rs:334-380),
 * so at byte granularity the 16 candidates [offset 0..3] x [NONE, SB, SH, SW] of the reference's select_store (store.rs:40-143) are lane
 * shuffles of two words — "SB at offset 1" is [y0, x0, y2, y3] — and its un-vendored splice_u8 / splice_u16 reduce to moving ciphertexts.
 * Zero-extending loads (LBU / LHU) are lane shuffles with ZERO lanes.  OUT OF SCOPE: sign-extending loads (LB / LH need bit operations
 * inside a byte) and the BDD circuits. */
/* GLWE `lane` of the word (kind, index); kind / index as fheram_select_src.  kind ZERO: an all-zero ciphertext, lane ignored. */
typedef struct fheram_select_lane { int32_t kind, index, lane, reserved /* 0 */; } fheram_select_lane;
/* fheram_bank_select with lane-mapped candidates.  lanes: [sum n_cand][word_size]; with L = lanes[(off_k + j) * word_size + w] for
 * select k, candidate j, word ciphertext w (off_k = the sum of the earlier n_cand)
 *     packed_{k,w} = glwe_normalize( sum_{j < n_cand[k]} X^j * source(L.kind, L.index)[L.lane] )     (one launch: k_select_pack_lanes)
 * and then exactly what fheram_bank_select runs: the selectors' digits prepared, the products, trace(0, log N), in the forms the bank's
 * configuration selects.  It IS the last select in every respect: fheram_bank_select_result, FHERAM_SRC_SELECT_RESULT and
 * fheram_bank_write_list_selected work on it unchanged, and it touches no member's rows, state flag, tree, result or kept memo; the last
 * read list's results stay readable.  With identity lanes (lane = w, one source per candidate) the outputs are int64-identical to
 * fheram_bank_select on the same sources; for any lanes, to fheram_bank_select on HOST candidates assembled from the downloaded sources.
 * The candidate pointers (up to 64 x 32) are a table in device memory, written by the host into a pinned buffer and copied by one
 * asynchronous copy on the bank's stream; a call waits for the host only where the previous lanes call's copy has not yet left the
 * pinned buffer (as host candidates do).  Table and pinned buffer are allocated on the first lanes call and freed with the bank
 * (FHERAM_ERR_DEVICE if that fails; every other operation still works).  fheram_bank_selftest_fail_select_alloc reaches the table's
 * device allocation as the one AFTER those the select's buffers ask for in the same call.
 * Refusals are fheram_bank_select's, checked for the whole call before anything is enqueued (a refused call changes nothing), and
 * FHERAM_ERR_INVALID_ARG also for: a lane outside [0, word_size) of a non-ZERO kind, reserved != 0.  HOST ciphertexts are range-checked
 * as there (FHERAM_ERR_RANGE), only the ciphertexts (slot, lane) a lane names. */
int fheram_bank_select_lanes(fheram_bank* bank, const fheram_selector* const* sels, const int* n_cand, int n,
                             const fheram_select_lane* lanes, const int64_t* host_words, int64_t* out /* [n][word_size][GLWE] or NULL */);
/* A FIELD SELECTOR: sum(widths) <= FHERAM_SELECT_BITS_MAX bits whose digit d has widths[d] bits at bit offset lsh_d = sum(widths[0..d)),
 * and may come from an integer and a bit position of its own (the store merge indexes by op + 4 * offset: two fields of two integers).
 * It is the Address of a one-row RAM of max_addr = 2^bits whose DECOMP_N starts with `widths` (get_base_2d then gives [widths], whatever
 * the bank's own DECOMP_N is): digit d is the GGSW of X^-(v_d << lsh_d) in the layout of address digits.  fheram_bank_select and
 * fheram_bank_select_lanes accept it; the selectors of one call share `bits` AND the digit count (the operand table has one stride).
 * FHERAM_ERR_INVALID_ARG: null pointers, n_fields outside [1, FHERAM_SELECT_FIELDS_MAX], a width < 1, a sum above
 * FHERAM_SELECT_BITS_MAX, n_ggsw != n_fields. */
#define FHERAM_SELECT_FIELDS_MAX 5
int fheram_bank_selector_alloc_fields(fheram_bank* bank, const int* widths, int n_fields, fheram_selector** out);
int fheram_bank_selector_create_fields(fheram_bank* bank, const int64_t* const* ggsw, int n_ggsw, const int* widths, int n_fields, fheram_selector** out);
/* digit d <- bits [first_bit[d], first_bit[d] + widths[d]) of fus[d] (n_fields integers, repeats allowed), in place: no allocation, no
 * host wait, through the unchanged k_cmux_chain — one launch per field.  Checked before anything is enqueued (FHERAM_ERR_INVALID_ARG):
 * null pointers, a selector or integer of another bank, a selector that no _fields call made, a field beyond its integer's width.
 * (fheram_bank_selector_derive refuses a field selector.) */
int fheram_bank_selector_derive_fields(fheram_bank* bank, fheram_selector* sel, const fheram_fheuint* const* fus, const int* first_bit);

/* ---- A step's addresses and selectors in ONE launch: the derive list.
 * *** CONTRACT-COMPATIBLE ONLY *** as fheram_address_derive and the select above: the same conversion (Address::set_from_fheuint,
 * conversion.rs:41-65), the same input type, the same digits.  fheram_address_derive_at issues one launch per distinct first_bit,
 * fheram_bank_selector_derive one per distinct (first_bit, bits) pair and fheram_bank_selector_derive_fields one per field, because their
 * kernel takes one digit plan for all its integers.  Here every item has an integer, a first bit and a sign of its own, and every output
 * digit is a job of a kernel that takes a flat list of them (k_cmux_jobs): any mix of addresses, selectors and selector fields is exactly
 * ONE launch of 6 * (digits over all items) workgroups.
 * Every digit is int64-identical to what fheram_bank_address_derive_at, fheram_bank_selector_derive or
 * fheram_bank_selector_derive_fields writes for the same integer, first bit, width and sign.  Targets are overwritten in place (from
 * _alloc, _create or an earlier derivation); no allocation, no host wait; the same integer may feed any number of items; mixed signs and
 * selector widths are allowed.  Ordering is that of the three calls: behind work of an earlier operation that still reads a named address,
 * every named address gets a fresh identity, later operations of the bank are ordered behind the launch.  The integers must stay alive
 * until the bank has been synchronised.
 * Checked for the whole list before anything is enqueued, a refused call changes no target.  FHERAM_ERR_INVALID_ARG: null items, n outside
 * [1, FHERAM_DERIVE_LIST_MAX], an unknown kind, a null or foreign integer or target, sign != 0 on a selector item, field != 0 on a
 * non-FIELD item, first_bit < 0 or the item's bits beyond the integer's width, an address or plain selector named twice, SELECTOR naming
 * a field selector or FIELD a plain one, field outside the selector's digits, a field selector of which the call names some digits but not
 * all or one digit twice, more than FHERAM_DERIVE_LIST_DIGITS_MAX digits in total.  FHERAM_ERR_UNSUPPORTED: an address plan of more
 * than 8 digits (as fheram_address_derive). */
enum { FHERAM_DERIVE_ADDRESS = 0,    /* target: fheram_addr*     — all digits of the bank's address plan from bits [first_bit, ..) of fu */
       FHERAM_DERIVE_SELECTOR = 1,   /* target: fheram_selector* — a plain selector's digits from bits [first_bit, first_bit + bits)     */
       FHERAM_DERIVE_FIELD = 2 };    /* target: fheram_selector* — digit `field` of a field selector from bits [first_bit, + widths[field]) */
typedef struct fheram_derive_item {
    int32_t kind, first_bit;
    int32_t sign;    /* ADDRESS: as fheram_address_derive; otherwise must be 0 (selectors are X^-v) */
    int32_t field;   /* FIELD: the digit; otherwise must be 0 */
    const fheram_fheuint* fu;
    void* target;
} fheram_derive_item;                       /* 32 bytes */
#define FHERAM_DERIVE_LIST_MAX 32           /* items per call */
#define FHERAM_DERIVE_LIST_DIGITS_MAX 64    /* digits over all items of a call (each is 6 workgroups) */
int fheram_bank_derive_list(fheram_bank* bank, const fheram_derive_item* items, int n);
/* the std-form digits of a bank address, [n_digits][fheram_ggsw_len]: the bank form of fheram_address_download (refuses an empty address) */
int fheram_bank_address_download(fheram_bank* bank, const fheram_addr* addr, int64_t* out);

/* ---- A bank's REGISTER FILE: a one-row RAM of 2^bits words that is read and written by selectors.
 * *** CONTRACT-COMPATIBLE ONLY *** as the select above.  A 32-word register file held as a bank member has the bank's shape and pays the
 * members' row chains on every access; but a select already IS Ram::read on a one-row RAM of max_addr = 2^bits whose row packs word j at
 * coefficient j.  A register file is that row made persistent, with a write side: its operations are Ram::read / read_prepare_write /
 * write (ram.rs:172-294, the rows == 1, one-coordinate path) of a RAM of max_addr = 2^bits, 1 <= bits <= FHERAM_SELECT_BITS_MAX, of
 * the bank's word_size.  Row w packs byte w of word j at coefficient j: [word_size][GLWE], what Ram::encrypt_sk of that RAM gives.
 * It lives on a bank beside the members, under the bank's keys, stream, configuration and round-off monitor.  Its addresses are the
 * bank's selectors — accepted when the selector belongs to the bank, is not empty and has bits == fheram_regs_bits(regs); plain and
 * field selectors alike — so rs1, rs2 and rd come out of the instruction word in the derive list's one launch.  Its results feed the
 * selects, and a write takes its word from any source kind.  No member's rows, state flag, tree, result or kept memo changes; the last
 * read list's and the last select's results stay readable; selects, read lists and member operations may run between
 * read_prepare_write and write, and a member between its own two halves resumes exactly as before.  fheram_bank_keys_load voids what a
 * register file kept for its write (the write then recomputes it).
 * Every check runs before anything is enqueued and a refused call changes nothing.  Common refusals — FHERAM_ERR_INVALID_ARG: null
 * arguments, a register file of another bank, a foreign or empty selector, a selector of other bits, an unknown source kind or a bad
 * index; FHERAM_ERR_UNINITIALIZED: no upload or pack yet; FHERAM_ERR_KEYS: keys not loaded; FHERAM_ERR_STATE: read, pack or
 * read_prepare_write between read_prepare_write and write, write outside it. */
typedef struct fheram_regs fheram_regs;
/* Every device buffer the register file will ever need is allocated here (the row, the kept trace, two temporaries, its prepared and
 * inverse digits); what the bank's register files share (the buffers of a read of FHERAM_SELECT_MAX outputs, the result and host-word
 * staging) by the bank's first create.  No operation allocates afterwards.  FHERAM_ERR_DEVICE if an allocation fails (the bank is as it
 * was).  A bank may hold any number of register files.
 * Who frees: fheram_regs_destroy frees the register file's device buffers while its bank lives.  fheram_bank_destroy frees the device
 * buffers of every register file still alive and detaches it; such a handle is then good for fheram_regs_destroy only, which releases
 * it.  Either order is safe.  Destroying the register file whose read_prepare_write was the bank's last voids FHERAM_SRC_REGS_OLD. */
int fheram_bank_regs_create(fheram_bank* bank, int bits, fheram_regs** out);
/* A WIDE register file: the same object with 1 <= bits <= FHERAM_TABLE_BITS_MAX, so up to 4096 words — a stack, a CSR
 * block, a scratch buffer or the data memory of a small program beside members of any shape.  It is the one-row RAM of max_addr =
 * 2^bits and every call below takes it unchanged; with bits > FHERAM_SELECT_BITS_MAX its addresses are WIDE selectors
 * (fheram_bank_table_selector_alloc / _create / _alloc_fields, up to FHERAM_SELECTOR_WIDE_DIGITS_MAX digits) under the same rule:
 * the selector's bits equal the register file's.  The buffers are those of fheram_bank_regs_create (the digit buffers hold
 * FHERAM_SELECTOR_WIDE_DIGITS_MAX digits either way).  fheram_bank_regs_create keeps its own bound.  What stays narrow:
 * fheram_bank_regs_pack holds at most min(2^bits, 32) candidates (fheram_bank_regs_load_plain / _encrypt_sk / _upload fill a whole
 * row, fheram_bank_regs_poke places single words), and fheram_bank_select / _select_lanes refuse a wide selector. */
int fheram_bank_regs_create_wide(fheram_bank* bank, int bits, fheram_regs** out);
void fheram_regs_destroy(fheram_regs* regs);
int fheram_regs_bits(const fheram_regs* regs);
/* 1 between read_prepare_write and write */
int fheram_bank_regs_state(const fheram_bank* bank, const fheram_regs* regs);
/* row: [word_size][GLWE] host int64.  Upload is range-checked as fheram_bank_ram_upload is (FHERAM_ERR_RANGE), makes the register file
 * readable, sets state 0 and voids anything kept — also between read_prepare_write and write, as fheram_bank_ram_upload. */
int fheram_bank_regs_upload(fheram_bank* bank, fheram_regs* regs, const int64_t* row);
int fheram_bank_regs_download(fheram_bank* bank, const fheram_regs* regs, int64_t* row);
/* row_w <- glwe_normalize( sum_{j < n_cand} X^j * source(srcs[j])[w] ), 1 <= n_cand <= min(2^bits, 32): exactly the pack of fheram_bank_select
 * (the same kernel, the same source checks) written into the register file; 2^bits ZERO sources give the all-zero register file with no
 * host encryption.  HOST slots are [0, 2^FHERAM_SELECT_BITS_MAX) of host_words, range-checked (FHERAM_ERR_RANGE).  Sets state 0; needs
 * no keys.  No host wait beyond the previous call's copy out of the pinned staging buffer. */
int fheram_bank_regs_pack(fheram_bank* bank, fheram_regs* regs, int n_cand, const fheram_select_src* srcs, const int64_t* host_words);
/* n independent Ram::read of the row as ONE operation, 1 <= n <= FHERAM_SELECT_MAX, n * word_size <= 64; all selectors share the digit
 * count.  The row is fanned out to the n * word_size chain inputs by one launch, then runs what fheram_bank_select runs behind its pack:
 * the digits prepared, the products, trace(0, log N), in the forms the bank's configuration selects.  out: [n][word_size][GLWE] or NULL
 * (no host wait; fheram_bank_regs_result later).  The row and the state flag do not change.  The outputs are the bank's "last register
 * read": FHERAM_SRC_REGS_RESULT names them until the next fheram_bank_regs_read of any register file of the bank. */
int fheram_bank_regs_read(fheram_bank* bank, const fheram_regs* regs, const fheram_selector* const* sels, int n, int64_t* out);
/* outputs [first, first + n) of the bank's last register read; FHERAM_ERR_STATE before any has run */
int fheram_bank_regs_result(fheram_bank* bank, int first, int n, int64_t* out);
/* Ram::read_prepare_write (ram.rs:196-222): the products with the selector's digits in place on the row (ram.rs:502-504), then
 * trace(0, log N) of the rotated row, which is the result — the OLD word — and is kept for the write (memo = 0: the write recomputes
 * it).  The state becomes 1.  out: [word_size][GLWE] or NULL (no host wait; fheram_bank_regs_old_result later).  The result is the
 * bank's FHERAM_SRC_REGS_OLD until the next fheram_bank_regs_read_prepare_write of any register file of the bank. */
int fheram_bank_regs_read_prepare_write(fheram_bank* bank, fheram_regs* regs, const fheram_selector* sel, int64_t* out);
int fheram_bank_regs_old_result(fheram_bank* bank, int64_t* out);
/* Ram::write (ram.rs:226-294) of ONE word taken on the device from `src` (any kind; HOST: slot src.index of host_words, range-checked as
 * write words are, FHERAM_ERR_RANGE — a refused word leaves the register file prepared and untouched): row <- normalize(row -
 * trace(row) + w), the selector's inverse digits, the products with them.  No host wait.  The state becomes 0.  Writing FHERAM_SRC_REGS_OLD
 * puts the old word back; `enable ? new : old` is a select over [REGS_OLD, HOST] whose output is written as FHERAM_SRC_SELECT_RESULT. */
int fheram_bank_regs_write(fheram_bank* bank, fheram_regs* regs, const fheram_selector* sel, fheram_select_src src, const int64_t* host_words);

/* ---- A bank's TABLES: read-only one-row RAMs of up to 4096 words, read by selectors — an instruction ROM, or a lookup table indexed
 * by an encrypted field.
 * *** CONTRACT-COMPATIBLE ONLY *** as the select and the register file above.  A row is one GLWE of N = 4096 coefficients, so a one-row
 * RAM holds up to 2^12 words; a program of a few thousand instructions held as a bank member has the bank's shape and pays the
 * members' row chains on every fetch.  A table is a one-row RAM of 2^bits words, 1 <= bits <= FHERAM_TABLE_BITS_MAX (= log N), of the
 * bank's word_size: its read is Ram::read (ram.rs:172-191, the rows == 1, one-coordinate path) of a RAM of max_addr = 2^bits.  Row w
 * packs byte w of word j at coefficient j: [word_size][GLWE], what Ram::encrypt_sk of that RAM gives.  It lives on a bank beside the
 * members and the register files, under the bank's keys, main stream, configuration and round-off monitor; it has no write side.
 * Its addresses are WIDE SELECTORS: ordinary fheram_selector handles of up to FHERAM_TABLE_BITS_MAX bits, made by the
 * fheram_bank_table_selector_* calls below (fheram_bank_selector_alloc / _create / _alloc_fields keep refusing more than
 * FHERAM_SELECT_BITS_MAX bits).  The plan is get_base_2d(2^bits) over the bank's DECOMP_N ([3,3,3,3] gives [3,3] [3,3,1] [3,3,2]
 * [3,3,3] [3,3,3,1] [3,3,3,2] [3,3,3,3] for bits = 6..12), or the caller's widths.  FHERAM_ERR_UNSUPPORTED: more than one coordinate, or
 * more than FHERAM_SELECTOR_WIDE_DIGITS_MAX digits.  fheram_bank_selector_derive, _derive_fields, fheram_bank_derive_list (SELECTOR and
 * FIELD items), _download, fheram_selector_n_digits and fheram_selector_destroy take a wide selector unchanged, so a fetch index is
 * bits [2, 2 + bits) of the pc in the derive list's one launch.  fheram_bank_select and fheram_bank_select_lanes refuse a selector of
 * more than FHERAM_SELECT_BITS_MAX bits (FHERAM_ERR_INVALID_ARG: their pack holds 32 candidates); a register file takes it by its
 * bits rule (a wide one: fheram_bank_regs_create_wide).
 * No member's rows, state flag, tree, result or kept memo changes, no register file's row or state; the last read list's, select's
 * and register read's results stay readable.  Every check runs before anything is enqueued and a refused call changes nothing.
 * FHERAM_ERR_INVALID_ARG: null arguments, a table or selector of another bank, an empty selector, a selector whose bits are not the
 * table's, selectors of different digit counts, n out of range, a wrong data_len; FHERAM_ERR_UNINITIALIZED: no upload or load yet;
 * FHERAM_ERR_KEYS: keys not loaded. */
#define FHERAM_TABLE_BITS_MAX 12          /* up to 4096 words: one per coefficient of the row */
typedef struct fheram_table fheram_table;
/* Every device buffer the table will ever need (the row: word_size GLWEs) is allocated here; what the bank's tables share (the buffers
 * of a read of FHERAM_SELECT_MAX outputs, the prepared digits of 8 selectors x 5 digits, the pinned result and the staging of
 * load_plain) by the bank's first create.  No operation allocates afterwards.  FHERAM_ERR_DEVICE if an allocation fails (the bank is
 * as it was).  A bank may hold any number of tables.
 * Who frees: as a register file.  fheram_table_destroy frees the table's row while its bank lives; fheram_bank_destroy frees the rows
 * of every table still alive and detaches it; such a handle is then good for fheram_table_destroy only, which releases it.  Either
 * order is safe. */
int fheram_bank_table_create(fheram_bank* bank, int bits, fheram_table** out);
void fheram_table_destroy(fheram_table* table);
int fheram_table_bits(const fheram_table* table);
/* row: [word_size][GLWE] host int64.  Upload is range-checked as fheram_bank_regs_upload is (FHERAM_ERR_RANGE) and makes the table
 * readable. */
int fheram_bank_table_upload(fheram_bank* bank, fheram_table* table, const int64_t* row);
int fheram_bank_table_download(fheram_bank* bank, const fheram_table* table, int64_t* row);
/* PUBLIC contents with no host encryption: data_len = 2^bits * word_size bytes in the layout fheram_ram_encrypt_sk takes (byte w of
 * word j at data[j * word_size + w]).  The row becomes the TRIVIAL ciphertext of those bytes: every mask limb 0, the body the plaintext
 * limbs Ram::encrypt_sk encodes (ram.rs:358-368) — int64-identical to fheram_ram_encrypt_sk of a RAM of max_addr = 2^bits with all-zero
 * mask and noise.  One kernel writes it from a pinned staging buffer; the only host wait is for the previous call's copy out of that
 * buffer.  Needs no keys and no secret.  Makes the table readable. */
int fheram_bank_table_load_plain(fheram_bank* bank, fheram_table* table, const uint8_t* data, size_t data_len);
/* n independent reads as ONE operation: entry k is Ram::read of tables[k] at sels[k].  The same table may be named several times and
 * several tables may share a call; 1 <= n <= FHERAM_SELECT_MAX, n * word_size <= 64; sels[k] has the bits of tables[k], and all
 * selectors of a call share the digit count (one stride of the operand table) — the tables of a call may differ in bits.  One launch
 * gathers row w of tables[k] to chain input k * word_size + w, then runs what fheram_bank_select runs behind its pack: the digits
 * prepared, the products, trace(0, log N), in the forms the bank's configuration selects.  out: [n][word_size][GLWE] or NULL (no host
 * wait; fheram_bank_table_result later).  The outputs are the bank's "last table read": FHERAM_SRC_TABLE_RESULT names them until the
 * next fheram_bank_table_read. */
int fheram_bank_table_read(fheram_bank* bank, const fheram_table* const* tables, const fheram_selector* const* sels, int n,
                           int64_t* out /* [n][word_size][GLWE] or NULL */);
/* outputs [first, first + n) of the bank's last table read; FHERAM_ERR_STATE before any has run */
int fheram_bank_table_result(fheram_bank* bank, int first, int n, int64_t* out);
/* WIDE selectors (header of this section): 1 <= bits <= FHERAM_TABLE_BITS_MAX; sum(widths) <= FHERAM_TABLE_BITS_MAX and
 * n_fields <= FHERAM_SELECTOR_WIDE_DIGITS_MAX.  Otherwise fheram_bank_selector_alloc / _create / _alloc_fields. */
int fheram_bank_table_selector_alloc(fheram_bank* bank, int bits, fheram_selector** out);
int fheram_bank_table_selector_create(fheram_bank* bank, const int64_t* const* ggsw, int n_ggsw, int bits, fheram_selector** out);
int fheram_bank_table_selector_alloc_fields(fheram_bank* bank, const int* widths, int n_fields, fheram_selector** out);

/* ---- THE PUBLIC SIDE of a bank: plain image loads, and one word read (peek) or written (poke) at a PUBLIC address.
 * *** CONTRACT-COMPATIBLE ONLY *** as the select, the register file and the tables are.  The server that hosts a bank has no secret
 * key: it loads a public program or data image, places input buffers and fetches result buffers at addresses everybody knows.  With a
 * public address a = r * N + q nothing is hidden, and the reference's operations collapse to row r: a read is "rotate row r by -q,
 * trace" (ram.rs:451,457 without the products), a write is write_first_step's normalize(a - b + c) (ram.rs:574-576) on that one row.
 * None of it pays the row chains over every row that an oblivious operation at a trivial GGSW address pays.
 * Everything runs on the bank's main stream.  The public side's buffers — two result buffers of min(FHERAM_PEEK_MAX * word_size, 64)
 * GLWEs (an operation writes the one that does not hold the last outputs), the gathered rows and a temporary of the same size, the
 * pinned result buffer, FHERAM_PEEK_MAX host-word slots and the byte staging buffers of one member — are allocated whole by the
 * first of these calls and freed with the bank (FHERAM_ERR_DEVICE if that fails; every other operation still works).  No later
 * operation allocates.  Every check runs before anything is enqueued and a refused call changes nothing. */
#define FHERAM_PEEK_MAX 16             /* entries of one peek or poke; n * word_size <= 64 as for the lists */
/* one more source kind: output `index` of the bank's last fheram_bank_peek or fheram_bank_poke; valid wherever a fheram_select_src or a
 * fheram_select_lane is taken (select, select_lanes, regs_pack, regs_write, poke, source_decrypt), FHERAM_ERR_STATE before any has run.
 * (Kind 9 is unknown, as kind 7 is: callers rely on both being refused with FHERAM_ERR_INVALID_ARG.) */
#define FHERAM_SRC_PEEK_RESULT 10
/* PUBLIC bytes into rows [first_row, first_row + n_rows) of one member with no host encryption and no int64 image: the rows become
 * the TRIVIAL ciphertexts Ram::encrypt_sk's encoding gives with an all-zero mask and zero noise (every mask limb 0, the body the
 * plaintext limbs of ram.rs:358-368), the rule of fheram_bank_table_load_plain.  data: the words [first_row * N, min(max_addr,
 * (first_row + n_rows) * N)) in the layout fheram_ram_encrypt_sk takes (byte w of word j at data[j * word_size + w]; sub-RAM w holds
 * byte w of every word, row r coefficient q holds word r * N + q); data_len = that word count * word_size; a ragged last row is
 * zero-padded.  The bytes are staged row by row into a pinned buffer, copied once and turned into rows by ONE launch (k_rows_plain);
 * the only host wait is for the previous plain load's copy out of the pinned buffer.  Needs no keys and no secret.
 * A whole-member load (first_row = 0, n_rows = fheram_rows) acts as fheram_bank_ram_upload does: the member becomes readable, its
 * state flag is cleared and whatever an earlier operation kept of its rows is void.  A row range needs a member that has rows
 * (FHERAM_ERR_UNINITIALIZED) and is not between read_prepare_write and write (FHERAM_ERR_STATE), and voids the same.
 * FHERAM_ERR_INVALID_ARG: no such member, null data, a row range that is empty or outside the member, a data_len that does not match. */
int fheram_bank_ram_load_plain(fheram_bank* bank, int member, size_t first_row, size_t n_rows, const uint8_t* data, size_t data_len);
/* the register file's twin: data_len = 2^bits * word_size bytes; acts as fheram_bank_regs_upload does */
int fheram_bank_regs_load_plain(fheram_bank* bank, fheram_regs* regs, const uint8_t* data, size_t data_len);
/* n reads at PUBLIC word addresses as ONE operation: with addrs[k] = r_k * N + q_k, for every word ciphertext y
 *     out_k[y] = trace(0, log N)( glwe_rotate(-q_k, rows[members[k]][y][r_k]) )
 * an encryption of [v, 0, .., 0], the form every read result has.  One launch gathers the n * word_size rotated ciphertexts
 * (k_peek_gather), then ONE trace runs over all of them in the form the bank's configuration selects (the single tail launch up to 8
 * ciphertexts).  1 <= n <= FHERAM_PEEK_MAX, n * word_size <= 64; members and addresses may repeat.  It changes no row, state flag,
 * tree, result slot or memo.  out: [n][word_size][GLWE] or NULL (no host wait; fheram_bank_peek_result later).  The outputs are the
 * bank's "last peek": FHERAM_SRC_PEEK_RESULT names them until the next fheram_bank_peek or fheram_bank_poke.
 * FHERAM_ERR_INVALID_ARG: null pointers, n or n * word_size out of range, a member outside the bank, an address >= max_addr;
 * FHERAM_ERR_UNINITIALIZED: a member without rows; FHERAM_ERR_KEYS: keys not loaded; FHERAM_ERR_STATE: a member between
 * read_prepare_write and write (its rows are rotated). */
int fheram_bank_peek(fheram_bank* bank, const int* members, const uint64_t* addrs, int n, int64_t* out /* [n][word_size][GLWE] or NULL */);
/* outputs [first, first + n) of the bank's last peek (or the old words of its last poke); FHERAM_ERR_STATE before any has run */
int fheram_bank_peek_result(fheram_bank* bank, int first, int n, int64_t* out);
/* n writes at PUBLIC word addresses as ONE operation: entry k writes the word srcs[k] names — any kind a select candidate may have,
 * HOST (slot index < FHERAM_PEEK_MAX of host_words) included, checked and staged as fheram_bank_regs_write checks and stages its
 * source — at addrs[k] of members[k].  All entries see the rows as they are before the call: for every touched (member, row r, word
 * ciphertext y), with j over the entries that fall in that row,
 *     R' = glwe_normalize( R - sum_j glwe_rotate(+q_j, t_j[y]) + sum_j glwe_rotate(+q_j, w_j[y]) )
 * where t_j is the peek of entry j, computed by the same gather and trace, and w_j the written word.  ONE more launch (k_poke_merge)
 * does the whole merge.  The t_j stay readable as the last peek — the OLD words, as read_prepare_write returns them
 * (fheram_bank_peek_result, FHERAM_SRC_PEEK_RESULT); a PEEK_RESULT source of the call itself names the outputs of the peek or poke
 * BEFORE it.  No host wait beyond the staging of host words.  What an earlier operation kept of the rows of every touched member is
 * void, as after an upload; untouched members and rows do not change.  The (member, address) pairs must be distinct.
 * Refusals as fheram_bank_peek's, and FHERAM_ERR_INVALID_ARG: null sources, a target named twice, an unknown source kind or index, a
 * HOST source with host_words == NULL; FHERAM_ERR_STATE: a source kind whose operation has not run, a MEMBER_RESULT member without a
 * result; FHERAM_ERR_RANGE: a host limb out of range. */
int fheram_bank_poke(fheram_bank* bank, const int* members, const uint64_t* addrs, int n, const fheram_select_src* srcs, const int64_t* host_words);
/* The register file's twins, narrow or wide: entry k is word idx[k] < 2^bits of the one row, which is address idx[k] of the one-row RAM
 * (row 0, coefficient idx[k]).  The same launches as above — one k_peek_gather, one trace over the n * word_size ciphertexts, and for
 * a poke one k_poke_merge on the one row — the same limits (FHERAM_PEEK_MAX entries, n * word_size <= 64, distinct targets of a poke),
 * the same source rules and host slots, and the same outputs: the bank's "last peek" (fheram_bank_peek_result,
 * FHERAM_SRC_PEEK_RESULT).  Both need keys, an initialised row (FHERAM_ERR_UNINITIALIZED) and state 0 (FHERAM_ERR_STATE: between
 * read_prepare_write and write the row is rotated).  A peek changes nothing else; a poke voids what the register file kept for a write.
 * FHERAM_ERR_INVALID_ARG: null pointers, a register file of another bank, n out of range, an index >= 2^bits, a target named twice. */
int fheram_bank_regs_peek(fheram_bank* bank, const fheram_regs* regs, const uint32_t* idx, int n, int64_t* out /* [n][word_size][GLWE] or NULL */);
int fheram_bank_regs_poke(fheram_bank* bank, fheram_regs* regs, const uint32_t* idx, int n, const fheram_select_src* srcs, const int64_t* host_words);
/* Self-test of the public side's FHERAM_ERR_DEVICE path, as fheram_bank_selftest_fail_select_alloc: the nth device allocation its
 * buffers ask for from now on fails once (0 withdraws the request). */
int fheram_bank_selftest_fail_public_alloc(fheram_bank* bank, int nth);

/* ---- MIXED READS: a read list, a table read and a register read of one bank as ONE operation.
 * *** CONTRACT-COMPATIBLE ONLY *** as its three parts are.  The reads of a VM step — the fetch from a table, rs1 / rs2 from the
 * register file, the data read of a member — take their addresses and selectors from one derive list launch and do not depend on each
 * other; as three calls each ends in its own pass through the latency-bound end of a read.  Here the groups go their own ways until
 * every ciphertext is a packed row and then share one top: with at most 8 ciphertexts whose digit counts are 0 or 2..4 that is ONE
 * launch (the products of every ciphertext and the trace), otherwise the products entry by entry and one trace over all of them.
 * A call names up to three groups, any of which may be empty (n = 0; its pointers are then not read) but not all three:
 *   list   members[n_list], addrs[n_list]        the rules of fheram_bank_read_list
 *   table  tables[n_table], table_sels[n_table]  the rules of fheram_bank_table_read (all selectors of the group share the digit count)
 *   regs   regs, reg_sels[n_regs]                the rules of fheram_bank_regs_read
 * with n_list + n_table + n_regs <= FHERAM_MIX_MAX and (n_list + n_table + n_regs) * word_size <= 64.  Every check runs before anything
 * is enqueued and a refused call changes nothing; each group is refused with the codes of its single call, the totals (and a null
 * argument, a negative count) with FHERAM_ERR_INVALID_ARG.
 * Entry k of a group is int64-identical to output k of that group's single call, and the bank is left exactly where the sequence
 * read_list(list), table_read(table), regs_read(regs) leaves it: FHERAM_SRC_LIST_RESULT / _TABLE_RESULT / _REGS_RESULT name the outputs
 * of their groups and fheram_bank_read_list_result / _table_result / _regs_result download them; the kinds of EMPTY groups keep their
 * last outputs; no row, state flag, tree, memo, select result or REGS_OLD changes, and a member or a register file between its two
 * halves resumes as before.  list_out / table_out / regs_out: [n][word_size][GLWE] of the group, each may be NULL; with all three NULL
 * the call waits for nothing.  The mix's buffers are allocated whole by the bank's first call (FHERAM_ERR_DEVICE if that fails). */
#define FHERAM_MIX_MAX 8
typedef struct fheram_mix_reads {
    const int* members;                        /* list: [n_list] */
    const fheram_addr* const* addrs;           /*       [n_list] */
    int n_list;
    const fheram_table* const* tables;         /* table: [n_table] */
    const fheram_selector* const* table_sels;  /*        [n_table] */
    int n_table;
    const fheram_regs* regs;                   /* regs: ONE register file */
    const fheram_selector* const* reg_sels;    /*       [n_regs] */
    int n_regs;
} fheram_mix_reads;
int fheram_bank_read_mix(fheram_bank* bank, const fheram_mix_reads* reads, int64_t* list_out, int64_t* table_out, int64_t* regs_out);
/* The reads of a step AND the first halves of its writes under ONE top.  *** CONTRACT-COMPATIBLE ONLY ***, as its parts
 * are.  A step's writes — the data memory's read_prepare_write, the register file's (rd) — take their address and selector from the same
 * derive list launch as its reads and end in a top of their own each; here the prepared ciphertexts join the reads' in one top, laid out
 * [list | table | regs | prepared list | prepared register file], and ONE launch behind it hands over what a read_prepare_write keeps.
 * The call is int64-identical to the sequence
 *   fheram_bank_read_mix(reads)                                    if reads names a read
 *   fheram_bank_read_prepare_write_list(members, addrs, n_list)    if n_list > 0
 *   fheram_bank_regs_read_prepare_write(regs, reg_sel)             if regs is not NULL
 * in every output and in everything that sequence leaves on the bank: rows, tree level 0, state flags and result slots of the members,
 * the register file's rotated row, state and kept trace (FHERAM_SRC_REGS_OLD), the read groups' last outputs (empty kinds keep theirs).
 * A member may be read and prepared in one call: its read sees the rows before the preparation; reads->regs may be prepares->regs: its
 * reads see the row before rd's products land in it.  Every later operation behaves as after the sequence, except that a prepare list of
 * ONE member starts no early inverse digits (a lone read_prepare_write does, on a bank of one member): its write computes them, as the
 * write after a list of several does.
 * All entries together — the reads, n_list and 1 for the register file — number at most FHERAM_MIX_MAX, and that total times word_size
 * at most 64.  Every check runs before anything is enqueued and a refused call changes nothing; each group is refused with the codes of
 * its single call, the totals, a null `prepares`, a negative count and a `prepares` that names nothing (that is fheram_bank_read_mix)
 * with FHERAM_ERR_INVALID_ARG.  reads == NULL: no reads.  list_out / table_out / regs_out: as fheram_bank_read_mix; prep_list_out:
 * [n_list][word_size][GLWE], the OLD words; prep_regs_out: [word_size][GLWE], the OLD register word; each may be NULL, with all five NULL
 * the call waits for nothing.  What the operation adds to the mix's buffers is allocated whole by the bank's first such call. */
typedef struct fheram_mix_prepares {
    const int* members;                 /* list: [n_list], the rules of fheram_bank_read_prepare_write_list (distinct members) */
    const fheram_addr* const* addrs;    /*       [n_list] */
    int n_list;
    fheram_regs* regs;                  /* regs: ONE register file and ONE selector (a register file has one pending write); NULL: none */
    const fheram_selector* reg_sel;
} fheram_mix_prepares;
int fheram_bank_read_prepare_write_mix(fheram_bank* bank, const fheram_mix_reads* reads, const fheram_mix_prepares* prepares,
                                       int64_t* list_out, int64_t* table_out, int64_t* regs_out, int64_t* prep_list_out, int64_t* prep_regs_out);

/* ---- Setup side of a bank: what "Setup side on the device" above is to a context, for a bank — so that a bank needs no
 * twin context and no host encryption — and the decryption of what a bank leaves on the device.  SAMPLING STAYS ON THE HOST, exactly as
 * there: the caller hands over mask limbs and noise polynomials, the same draws give the same ciphertexts.  Every call waits for the
 * device (both streams idle before and after).  Every check runs before anything is enqueued or staged: a refused call changes nothing.
 * (These declarations stand here and not beside the context's because they need the bank's handle types.) */
/* fheram_secret_create on the bank's context: the secret is bound to the bank, freed with fheram_secret_destroy; destroying the bank
 * first or the secret first are both safe. */
int fheram_bank_secret_create(fheram_bank* bank, const int64_t* sk, fheram_secret** out);
/* fheram_keys_encrypt_sk: the same keys from the same draws; afterwards everything fheram_bank_keys_load voids is void (what the members
 * and the register files kept for a write). */
int fheram_bank_keys_encrypt_sk(fheram_bank* bank, const fheram_secret* sk, const int64_t* mask, const int64_t* noise, int64_t* std_out);
/* fheram_address_encrypt_sk / fheram_fheuint_encrypt_sk: an ordinary bank address / integer. */
int fheram_bank_address_encrypt_sk(fheram_bank* bank, const fheram_secret* sk, uint32_t value, const int64_t* mask, const int64_t* noise,
                                   fheram_addr** out);
int fheram_bank_fheuint_encrypt_sk(fheram_bank* bank, const fheram_secret* sk, uint32_t value, int n_bits, const int64_t* mask,
                                   const int64_t* noise, fheram_fheuint** out);
/* fheram_glwe_encrypt_sk / fheram_glwe_decrypt on the bank's secret: the words of fheram_bank_write* and HOST candidates, and the
 * decryption of downloaded results. */
int fheram_bank_glwe_encrypt_sk(fheram_bank* bank, const fheram_secret* sk, int n_glwe, int size, int k, const int64_t* pt, int pt_size,
                                int pt_col, const int64_t* mask, const int64_t* noise, int64_t* out);
int fheram_bank_glwe_decrypt(fheram_bank* bank, const fheram_secret* sk, int n_glwe, int size, const int64_t* ct, int64_t* pt);
/* Ram::encrypt_sk (ram.rs:129-167) of ONE member, straight into its rows: data = max_addr * word_size bytes, mask
 * [word_size][rows][3][N], noise [word_size][rows][N] — int64-identical to fheram_ram_encrypt_sk on a context of the bank's
 * fheram_params.  The member ends as fheram_bank_ram_upload leaves it; every other member is untouched.  Refusals: fheram_ram_encrypt_sk's
 * ("invalid data: ..."), "no such member". */
int fheram_bank_ram_encrypt_sk(fheram_bank* bank, int member, const fheram_secret* sk, const uint8_t* data, size_t data_len,
                               const int64_t* mask, const int64_t* noise);
/* The row of a register file / a table: Ram::encrypt_sk for the one-row RAM of max_addr = 2^bits — byte w of word j at coefficient j,
 * zero behind word 2^bits - 1.  data = 2^bits * word_size bytes, mask [word_size][3][N], noise [word_size][N].  The object ends as
 * fheram_bank_regs_upload / fheram_bank_table_upload leave it. */
int fheram_bank_regs_encrypt_sk(fheram_bank* bank, fheram_regs* regs, const fheram_secret* sk, const uint8_t* data, size_t data_len,
                                const int64_t* mask, const int64_t* noise);
int fheram_bank_table_encrypt_sk(fheram_bank* bank, fheram_table* table, const fheram_secret* sk, const uint8_t* data, size_t data_len,
                                 const int64_t* mask, const int64_t* noise);
/* Fills an existing selector of any kind (plain, fields, wide; empty or not: overwritten like a derivation) with the digits
 * Address::encrypt_sk (address.rs:86-109) gives for the one-row RAM of max_addr = 2^bits over the plan the handle stores: digit d = GGSW
 * of X^-(((value >> rsh_d) mod 2^width_d) << lsh_d).  mask [n_digits][3][2][4][N], noise [n_digits][3][2][N], digit-major.
 * FHERAM_ERR_INVALID_ARG: value >= 2^bits, a selector or secret of another bank. */
int fheram_bank_selector_encrypt_sk(fheram_bank* bank, const fheram_secret* sk, fheram_selector* sel, uint32_t value, const int64_t* mask,
                                    const int64_t* noise);
/* Decrypts and decodes, ON THE DEVICE (k_decrypt_decode), coefficient 0 of the word_size ciphertexts of each of n words named as a
 * select's candidates are — kinds MEMBER_RESULT, LIST_RESULT, SELECT_RESULT, REGS_RESULT, REGS_OLD, TABLE_RESULT (HOST and ZERO:
 * FHERAM_ERR_INVALID_ARG); n * word_size <= 64.  want [n][word_size] or NULL (the decoded value itself is the expectation); values
 * [n][word_size]: decode_coeff_i64 / 2^(k - k_pt), rounded half away from zero; log2_noise [n][word_size] or NULL: log2|res - (want <<
 * (k - k_pt))| - k (-inf for 0), the example's metric (examples/fhe-ram.rs:224-237).  No result buffer, row, state flag or memo changes. */
int fheram_bank_source_decrypt(fheram_bank* bank, const fheram_secret* sk, const fheram_select_src* srcs, int n, const int64_t* want,
                               int64_t* values, double* log2_noise);
/* The same for every data coefficient of every row of a member / a register file / a table: values = max_addr * word_size (2^bits *
 * word_size) int32 in the interleaved order of the encrypting call's data; worst_log2_noise (may be NULL): the maximum over them of the
 * metric against each coefficient's own decoded value — the margin to a decode failure.  FHERAM_ERR_UNINITIALIZED: no rows yet;
 * FHERAM_ERR_STATE: between read_prepare_write and write (the rows are rotated).  Rows, state and memos are unchanged. */
int fheram_bank_ram_decrypt(fheram_bank* bank, int member, const fheram_secret* sk, int32_t* values, double* worst_log2_noise);
int fheram_bank_regs_decrypt(fheram_bank* bank, const fheram_regs* regs, const fheram_secret* sk, int32_t* values, double* worst_log2_noise);
int fheram_bank_table_decrypt(fheram_bank* bank, const fheram_table* table, const fheram_secret* sk, int32_t* values, double* worst_log2_noise);

/* ---- Measurement hooks (bench.py).  HIP events recorded on the context's own stream. */
int fheram_timer_begin(fheram_ctx* ctx);
int fheram_timer_end(fheram_ctx* ctx, float* elapsed_ms);
/* Per-kernel-class timing: when enabled, every launch of the hot kernels is bracketed by HIP
 * events on the launch stream; totals are read back per class name
 * ("ext_product", "keyswitch", "prepare", "elementwise").  on = 2: only the chain launches themselves
 * ("keyswitch_chain_launch": two events per launch of the dominant kernel, nothing else — back-to-back submission of
 * the other launches stays as in an unprofiled run). */
int fheram_profile_enable(fheram_ctx* ctx, int on);
int fheram_profile_get(fheram_ctx* ctx, const char* kernel_class, uint64_t* launches, uint64_t* blocks, double* total_ms);
int fheram_profile_reset(fheram_ctx* ctx);
/* The trace chain at the end of a read (ram.rs:457,540) runs as one launch whose workgroups hand over inside the
 * kernel; a launch that could not assemble its workgroup groups (CUs held by another context) gives up and the fused
 * launch enqueued behind it redoes the chain, with the same result.  launches = such launches since the context was
 * created, fallbacks = how many of them gave up.  Waits for the context's stream. */
int fheram_tail_stats(fheram_ctx* ctx, uint64_t* launches, uint64_t* fallbacks);
/* The same for the dependent chains on 9..64 ciphertexts (the alone packer levels, CoordinatePrepared::product[_inplace]
 * and write_mid_step's traces at MAX_ADDR = 2^14 — the source default — to 2^16), which run as one launch with in-kernel
 * hand-offs too (k_chain_mid).  Each ciphertext's workgroups stand alone there: fallbacks = CIPHERTEXTS redone by the fused
 * launch behind (0 on a GPU the context has to itself). */
int fheram_mid_stats(fheram_ctx* ctx, uint64_t* launches, uint64_t* fallbacks);
/* enabled: the FHERAM_MID setting in effect (0 = the path has switched the single-launch mid chains off because their launches kept
 * giving up — two windows of 64 launches in a row with more than a quarter of the ciphertexts redone — and will try them again
 * 256 ops later); times_disabled: how often that has happened on this context */
int fheram_mid_state(const fheram_ctx* ctx, int* enabled, uint64_t* times_disabled);
/* BASELINE.json configs[1]: one GLWE x GGSW external product at N = 4096 on device-resident synthetic
 * operands (normalised limbs; the work is data independent).  Runs `iters` launches of `batch` products
 * back to back on the context's stream, each launch consuming the previous one's output (a dependent
 * chain, as CoordinatePrepared::product is, coordinate_prepared.rs:147-161), and returns the HIP-event
 * time of the whole chain in ms.  batch = 1 gives the latency of one product, batch >= #CUs the throughput. */
int fheram_bench_external_product(fheram_ctx* ctx, int batch, int iters, float* total_ms);
/* The two dependent chains that carry the path's work, on device-resident synthetic operands, `iters` times back to back:
 * kind 0 = GLWE::trace(0, n) on `batch` ciphertexts (the packer levels in which a row is alone, ram.rs:514, and
 * write_mid_step's traces, ram.rs:616,621), kind 1 = CoordinatePrepared::product over n digits (coordinate_prepared.rs:147-177).
 * Returns the HIP-event time of all iterations in ms. */
int fheram_bench_chain(fheram_ctx* ctx, int kind, int batch, int n, int iters, float* total_ms);
/* Device properties of the context's GPU (name, CU count) for the bench report. */
int fheram_device_info(const fheram_ctx* ctx, char* name, size_t name_len, int* compute_units);

/* ---- Self-test of the arithmetic the kernels are built on (no reference counterpart: the reference delegates its
 * arithmetic to Poulpy's FFT64 backend, examples/fhe-ram.rs:3-7, whose contract — the FP64 round-off of a product of
 * normalised limbs stays below 1/2, so rounding gives the exact integer — is the contract of csrc/fft_dev.hpp too).
 * n_terms (even, <= 8) pairs of polynomials of N int32 coefficients in; out[0][N] = sum_r a_r * g_r and
 * out[1][N] = sum_r a_r * g_{r ^ 1} (negacyclic) as RAW doubles, BEFORE the rounding the path applies, through the
 * transforms, the prepared-operand scaling and the multiply-accumulate exactly as the fused kernels call them
 * (singles != 0: every transform on its own instead of two at a time).  The caller compares with exact integer arithmetic
 * (tests/test_gpu_fft.py).  Not on the RAM path. */
int fheram_selftest_convolve(fheram_ctx* ctx, int n_terms, const int32_t* a, const int32_t* g, double* out, int singles);
/* The same products with the ROUNDING of the path (nat_out) and therefore through the round-off monitor: out = the rounded
 * sums.  operand_scale multiplies the prepared operands (1.0: the path's arithmetic; 0.5 makes every odd sum a half-integer,
 * which is how tests/test_gpu_fft.py drives the monitor over its limit and checks FHERAM_ERR_PRECISION). */
int fheram_selftest_convolve_rounded(fheram_ctx* ctx, int n_terms, const int32_t* a, const int32_t* g, double* out, double operand_scale);
/* Self-test of the limb arithmetic (csrc/limb_forms.hpp: the limb walk, rsh(1) and the closed-form normalisation of the chain
 * kernels, as the scalar functions the kernels call).  One coefficient of `form` (csrc/limb_forms_eval.hpp: LimbForm, 0..13)
 * per thread: in[n][10] and out[n][6] doubles holding exact integers, n <= 2^20; outputs a form does not produce are 0.
 * The caller compares with exact integer arithmetic (tests/test_gpu_limb_forms.py).  Not on the RAM path. */
int fheram_selftest_limb_forms(fheram_ctx* ctx, int form, int n, const double* in, double* out);
/* Self-test of EVERY transform form the kernels call (csrc/selftest.hpp: SelftestForm), each under the buffer discipline of its call
 * sites: the forward transforms one, two or three at a time (fwd_polys), and inv_form =
 *   0 fft_inv_skew<1, 1>    1 fft_inv_skew<2, 1>    2 fft_inv_skew<1, 0> on alternating buffers    3 fft_inv_skew<1, 0> behind a forward
 *   transform in the same buffer    4 fft_inv_skew<1, 2>    5 fft_inv_skew<2, 2>    6 fft_inv1_hooked<2> twice per batch in one buffer
 *   7 fft_inv2_hooked<2>    8 pair, pair, two singles, pair: both hooked forms in the same buffers under one free counter.
 * a, g: [n_batches][n_terms][N] int32 (n_terms even, <= 8; 1 <= n_batches <= 4); out: [n_batches][2][N] doubles, per batch the two
 * sums of fheram_selftest_convolve.  One workgroup transforms the batches one after the other in the same exchange buffers and takes
 * batch i + 1's products while batch i is transformed (inside the hooks of forms 6..8), so a race in the reuse of the buffers shows
 * as a batch that differs from the same operands run alone.  Every form computes the same doubles: inv_form 1 with one batch
 * is fheram_selftest_convolve bit for bit.  rounded = 0: raw doubles; rounded != 0: the path's rounding, through the round-off
 * monitor, with FHERAM_ERR_PRECISION as fheram_selftest_convolve_rounded returns it (operand_scale as there).  spectra (may be NULL):
 * [2][n_batches][n_terms][N] doubles, the transform-domain a and the prepared g as the forward launch left them.
 * The caller compares with exact integers and across forms (tests/test_gpu_fft_forms.py).  Not on the RAM path. */
int fheram_selftest_forms(fheram_ctx* ctx, int fwd_polys, int inv_form, int n_terms, int n_batches, const int32_t* a, const int32_t* g, double* out,
                          int rounded, double operand_scale, double* spectra);

#ifdef __cplusplus
}
#endif
#endif /* FHERAM_H */
