// Private to the C-ABI library (one translation unit, fheram.hip): context / address / secret objects,
// error and profiling helpers, the int64 <-> int32 layout conversion at the boundary.
#pragma once
#include "../../include/fheram.h"
#include "kernels.hpp"
#include "cmux_chain.hpp"
#include "cmux_jobs.hpp"
#include "mapped_chains.hpp"
#include "tail_wait.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace fk;

namespace {

thread_local std::string g_create_err;

// Twiddle table of the transforms: fk::make_fft_twiddles() (fft_dev.hpp).

struct ProfCls {
    uint64_t launches = 0, blocks = 0;
    double ms = 0.0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

}  // namespace

inline uint64_t next_addr_id() { static std::atomic<uint64_t> n{0}; return ++n; }

// What ONE RAM carries from one operation to the next: a context holds one, a bank one per member (bank.hpp), and an operation updates
// the one its operand set names (path.hpp Opnds::st).
struct RamState {
    bool initialized = false, state = false;
    // Results of read_prepare_write that Ram::write recomputes on the unchanged state (FHERAM_MEMO=0 recomputes them):
    //  memo_top  : d_trtop = trace(tree top) — the output of read_prepare_write (ram.rs:540) is the very value
    //              write_first_step computes first (ram.rs:571-572: same ciphertext, same deterministic operations);
    //  memo_alone: arena A holds every local row after the packer levels in which it is alone (ram.rs:514; n steps),
    //              which ARE the first n steps of trace(ct_hi) in write_mid_step (ram.rs:616).
    bool memo_top = false;
    int memo_alone = 0;
    bool res_in_trtop = false;   // the last read / read_prepare_write left its result in d_trtop (else d_res)
};

// The DENSE buffers of an operation on several addresses that does not run in place: every per-ciphertext and per-row buffer of a RamView
// (path.hpp) but the rows, for `cap` addresses of ws ciphertexts.  Ciphertext y = k * ws + w is word w of address k; the arenas keep the
// rows' stride (sy = rows * GLWE).  Three owners: fheram_read_batch (the context's `batch`), fheram_bank_read_list and the bank's
// read_prepare_write / write lists (bank.hpp; sized by the members' word count, not by the context's, which is the whole bank's).
// Allocated on first use with what the owner's operations need (path.hpp dense_reserve), grown to the largest operation seen, freed with
// the owner; every launch of such an operation writes these only (path.hpp dense_view).
struct DenseBufs {
    int cap = 0;
    int32_t *A = nullptr, *B = nullptr, *C = nullptr, *D = nullptr;   // [cap * ws][rows]  reads: A and B from the first operation of several addresses on, C only where the alone levels run as the tail chain (path.hpp third_arena_needed), never D
    int32_t *part = nullptr, *tmp = nullptr, *tmp2 = nullptr, *res = nullptr, *tree = nullptr, *w = nullptr, *trtop = nullptr;   // [cap * ws]  reads: res, and tmp / tmp2 with A and B
    double* prep = nullptr;               // [cap][n_digits] prepared GGSW, address k's digits: reads only, with A and B (a bank's write lists use the bank's tables)
    int64_t *h_res = nullptr, *d_h_res = nullptr;   // reads only — pinned, device-visible: the results as int64 (+ the monitor's maximum), as fheram_ctx::h_res
};

// ---- the execution switches (include/fheram.h fheram_config): two pure host functions, no HIP call in them -------------------------------
// The library defaults, without the environment (fheram_config_default adds the FHERAM_* overrides; a context's cfg starts from these).
inline fheram_config config_builtin() {
    fheram_config d{};
    d.limb_split = 1; d.fine_split = 1; d.memo = 1; d.pre_inv = 1; d.tail = 1; d.tail_test = 0; d.mid = 2; d.mid_test = 0;
    d.chain = 1; d.chain_y = 3; d.pair_z = 1; d.fuse = 1; d.graph = 0; d.safe = 0; d.nco = 0; d.tail_ep = 1; d.monitor = 1; d.reserved = 0;
    return d;
}
// The switches IN EFFECT for a requested configuration: every field clamped to its values, then what `memo`, `graph` and `safe` imply for
// the others, in this order (graph zeroes pre_inv before safe looks at it).  reserved comes out 0: fheram_ctx_create_cfg has refused anything else.
inline fheram_config config_in_effect(const fheram_config& in) {
    using C = fheram_config;
    fheram_config e{};
    for (int32_t C::*on_off : {&C::limb_split, &C::fine_split, &C::memo, &C::tail, &C::tail_ep, &C::mid_test, &C::chain, &C::pair_z, &C::fuse, &C::graph, &C::safe})
        e.*on_off = in.*on_off ? 1 : 0;
    for (int32_t C::*upto2 : {&C::tail_test, &C::mid, &C::monitor}) e.*upto2 = in.*upto2 < 0 ? 0 : (in.*upto2 > 2 ? 2 : in.*upto2);   // mid = 1: the <= 16 ciphertext split only
    e.chain_y = in.chain_y ? 3 : 0;
    e.nco = in.nco == 2 ? 2 : (in.nco == 1 ? 1 : 0);
    e.pre_inv = e.memo ? (in.pre_inv == 2 ? 2 : (in.pre_inv ? 1 : 0)) : 0;
    // a captured launch sequence must be a pure function of (context, address, op): under replay the write always
    // computes its own inverse digits (whether a precompute matched is state the capture would freeze)
    if (e.graph) e.pre_inv = 0;
    // safe: ONE switch for a configuration that stays inside the HIP memory model — no launch with in-kernel hand-offs
    // between workgroups (k_trace_tail, k_chain_mid: relaxed agent-scope atomics + drained stores + L1-bypassing loads on one
    // XCD's L2) and no gate wave (k_tail_gate): dependent steps are kernel boundaries, the side work forks from an event.
    // Same results (tests/test_gpu_golden.py); priced in profiles/r05_bench_safe.json.
    if (e.safe) { e.tail = 0; e.tail_test = 0; e.mid = 0; e.mid_test = 0; if (e.pre_inv == 1) e.pre_inv = 2; }
    // round-off monitor: one coefficient per thread and transform by default, every coefficient under `safe`
    if (e.safe && e.monitor == 1) e.monitor = 2;
    return e;
}

// Every device allocation, pinned host allocation and event a context makes (its bank's operand tables included), recorded as it is made:
// release() gives all of them back, so nothing that allocates has a second line to remember.  Each helper returns the HIP call's status and records
// only what succeeded (a failed call's pointer stays null).  No destructor: fheram_ctx_destroy calls release() on the context's device, streams drained.
struct CtxResources {
    std::vector<void*> dev, pinned;
    std::vector<hipEvent_t> events;
    template <typename T> hipError_t device(T** p, size_t bytes) { const hipError_t e = hipMalloc((void**)p, bytes); if (e == hipSuccess) dev.push_back(*p); return e; }
    template <typename T> hipError_t host(T** p, size_t bytes, unsigned flags) { const hipError_t e = hipHostMalloc((void**)p, bytes, flags); if (e == hipSuccess) pinned.push_back(*p); return e; }
    hipError_t event(hipEvent_t* ev, bool timing = false) {   // ordering events carry no time stamps
        const hipError_t e = timing ? hipEventCreate(ev) : hipEventCreateWithFlags(ev, hipEventDisableTiming);
        if (e == hipSuccess) events.push_back(*ev);
        return e;
    }
    void release() {
        for (hipEvent_t e : events) hipEventDestroy(e);
        for (void* p : dev) hipFree(p);
        for (void* p : pinned) hipHostFree(p);
        events.clear(); dev.clear(); pinned.clear();
    }
};

struct fheram_ctx {
    // ---- parameters, and what is derived from them (never changed after creation) ----
    fheram_params p;
    int device = 0;
    int ws = 0, n2 = 0, n_digits = 0, max_digits = 0;
    size_t rows = 0;        // GLWE rows per sub-RAM held by THIS context (all of them unless sharded)
    size_t rows_glob = 0;   // rows per sub-RAM of the whole RAM
    int shard = 0, n_shards = 1;   // row sharding: this context owns rows r = shard (mod n_shards)
    std::vector<std::vector<int>> base2d;
    static constexpr int S_CT = 3, S_ADDR = 4, S_INV = 5, DNUM_CT = 3, DNUM_GGSW = 4;
    int s_evk = 4;          // limbs of a trace / packing key: ceil(k_evk_trace / base2k) = 4 (source constants, parameters.rs:17) or 5 (README.md:17-27: K_EVK = 5 * BASEK)
    size_t atk = 0;         // elements of one trace key: DNUM_CT * s_evk * 2 * N   (evk_glwe_infos, parameters.rs:71-81)
    static constexpr size_t GLWE = (size_t)S_CT * 2 * N;                   // elements of a ct
    static constexpr size_t GLWE4 = (size_t)S_ADDR * 2 * N;                // one GGSW row ct
    static constexpr size_t GGSW = (size_t)DNUM_CT * 2 * GLWE4;            // elements of a GGSW
    static constexpr size_t EVK5 = (size_t)DNUM_GGSW * S_INV * 2 * N;      // inverse / tensor key
    static constexpr size_t GGSW5 = (size_t)DNUM_GGSW * 2 * S_INV * 2 * N; // one bit of an FheUint (N4)
    int cus = 256;
    CtxResources res;       // every buffer and event below but the streams and `batch`: allocated through it, freed by its release()
    // ---- streams and ordering events ----
    hipStream_t stream = nullptr;    // main stream: every op is ordered on it
    hipStream_t stream2 = nullptr;   // side stream for work that is independent inside one op (write path)
    hipStream_t cur = nullptr;       // stream the launchers currently enqueue on
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_xout = nullptr, ev_xin = nullptr;   // ordering against a caller's stream (fheram_stream_signal / _wait)
    // ---- the execution switches IN EFFECT (config_in_effect of what the caller asked for; include/fheram.h describes each).  After
    //      creation only the two watches below write one: cfg.tail (off for good) and cfg.mid (off, re-armed after 256 ops) ----
    fheram_config cfg = config_builtin();
    bool wide = false;             // the launch being enqueued can never meet the gate wave (Ram::read, Ram::write: only read_prepare_write parks one): the chain kernels' 256-register variants
    // ---- keys and tables ----
    double* d_tw = nullptr;
    double ninv = 0.0;
    double* d_atk = nullptr;       // [log_n] prepared trace keys
    double* d_atk_inv = nullptr;
    double* d_tsk = nullptr;
    int64_t gal[LOGN];
    bool keys_loaded = false;
    //  Round-off monitor (fft_dev.hpp mon_note / RoMonitor; cfg.monitor): every rounding of an inverse transform reports |x - rint(x)|; the
    //  context's maximum lives behind its twiddle table (d_tw[N]), and a pinned host word is set once it passed MON_LIMIT.
    unsigned* h_ro_flag = nullptr; // pinned, device-visible: 1 = a round-off above MON_LIMIT was seen (sticky until fheram_roundoff_reset)
    // ---- the RAM: the buffers indexed by ciphertext (the sequences of path.hpp reach them through a RamView only) ----
    int32_t* d_data = nullptr;     // [ws][rows] GLWE
    int32_t* d_tree = nullptr;     // [ws] GLWE (tree[0][0])
    int32_t* d_scrA = nullptr;     // [ws][rows]  ping-pong arenas: every fused kernel is out of place
    int32_t* d_scrB = nullptr;     // [ws][rows]
    int32_t* d_scrC = nullptr;     // [ws][rows]
    int32_t* d_scrD = nullptr;     // [ws][rows]
    int32_t* d_res = nullptr;      // [ws]
    int32_t* d_tmp = nullptr;      // [ws]
    int32_t* d_tmp2 = nullptr;     // [ws]
    int32_t* d_w = nullptr;        // [ws]
    int32_t* d_trtop = nullptr;    // [ws]
    int32_t* d_part = nullptr;     // [ws]            this shard's partial pack / the un-rotated ct_lo
    int32_t* d_gat[3] = {nullptr, nullptr, nullptr};   // [n_shards][ws] gathered partials + ping-pong (root)
    RamState ram;                  // this context's RAM (a bank's context: unused, the members' are in fheram_bank)
    DenseBufs batch;               // fheram_read_batch: its arenas, results and digit table (path.hpp dense_reserve / dense_view), sized by this context's word count
    // ---- launcher scratch ----
    double* d_big = nullptr;       // [LIMB_SPLIT_MAX ciphertexts] un-normalised limbs of the limb-parallel path
    double* d_big2 = nullptr;      // same, for launches on the side stream
    double* d_prep = nullptr;      // [n_digits] prepared GGSW: coordinate ci at its first digit (write: inverse digits at 0)
    bool prep1_ready = false;      // coordinate 1 was prepared together with coordinate 0 (unsharded reads)
    int32_t* d_ggsw_tmp = nullptr; // [max digits per coordinate] std GGSW (inversion result)
    int32_t* d_ggsw_tmp2 = nullptr;
    // ---- tail (cfg.tail): the dependent trace chain at the end of a read as ONE launch with in-kernel hand-offs (k_trace_tail);
    //      cfg.tail_test: every launch gives up two steps before its end and the fused fallback launch behind it does the work ----
    unsigned tail_seq = 0;
    int tail_xoff = 0;                 // first XCD of this context's groups (0 or 4, alternating over contexts and processes)
    uint64_t tail_launches = 0;
    //  watch: the fallback launch mirrors its count into a pinned host word; if more than a quarter of the last 64
    //  single-launch chains gave up (a GPU shared so heavily, or partitioned so, that their groups do not fit side by
    //  side: each such launch waited ~5 ms first), the context goes back to one launch pair per step for good.
    unsigned* h_tail_fb = nullptr;     // pinned, device-visible
    unsigned tail_fb_mark = 0;
    uint64_t tail_launch_mark = 0;
    unsigned* d_tail_sync = nullptr;   // [8 groups][32] + abort generation, fallbacks taken, gate, groups gone
    //  done words: the tail's last workgroup to leave tells the host so (tail_wait.hpp): fheram_sync ends on them when a read-type
    //  operation's tail and its predicated fallback are the last thing on the main stream, instead of on the end of both kernels
    unsigned* h_tail_done = nullptr;   // pinned, device-visible: [0] done, [16] gave up
    unsigned* d_h_tail_done = nullptr; // device address of h_tail_done
    TailWait tail_wait;
    // ---- mid (cfg.mid): dependent chains on 9..64 ciphertexts as ONE launch with in-kernel hand-offs (k_chain_mid); cfg.mid_test: every
    //      launch gives up late.  One sync block per stream ----
    unsigned mid_seq = 0;
    uint64_t mid_launches = 0, mid_launch_mark = 0;
    unsigned mid_fb_mark = 0;
    int mid_bad_windows = 0, mid_saved = 0;          // auto-disable of the single-launch mid chains: consecutive bad windows; the setting to come back to
    uint64_t mid_window_cts = 0, mid_disabled_count = 0; // ciphertexts launched in the current window of 64 launches; times the path has been switched off
    unsigned mid_off_ops = 0;                        // ops since then (re-armed after 256: launch.hpp mid_rearm)
    unsigned* h_mid_fb = nullptr;      // pinned, device-visible: ciphertexts redone, [0] main stream, [16] side stream
    unsigned* d_mid_sync[2] = {nullptr, nullptr};   // [64 groups][32] + [_, ciphertexts redone]: main / side stream
    double* d_mid_big[2] = {nullptr, nullptr};      // [step parity][ciphertext x RS <= 64] x BIG_STRIDE doubles: k_chain_mid's partial limb polynomials
    double* d_mid_y[2] = {nullptr, nullptr};        // [2][64 groups][2][N] doubles: the chain's intermediates in the one-double form
    // ---- the inverse-digit precompute (cfg.pre_inv) ----
    //  inv_id[ci]: d_prep_inv holds the prepared INVERSE digits of coordinate ci of the address with that id
    //              (CoordinatePrepared::prepare_inv, ram.rs:260-271,278-289): read_prepare_write — which is told the
    //              address the write will use — starts them on the (low-priority) side stream next to its trace chain,
    //              which is one launch holding 24 CUs on half of the XCDs: the rest of the chip is idle then.  A write
    //              with another address, or after new keys, computes them itself.  FHERAM_PRE_INV=0: always.
    uint64_t inv_id[2] = {0, 0};
    double* d_prep_inv = nullptr;  // [n_digits] prepared GGSW
    int32_t* d_ggsw_inv = nullptr; // [n_digits] std GGSW: the inversion result on its way there (own scratch: runs beside anything)
    hipEvent_t ev_inv[2] = {nullptr, nullptr};
    bool inv_pending[2] = {false, false};   // a precompute of coordinate ci has been enqueued on the side stream and no write has consumed / overwritten it
    hipEvent_t ev_wdone = nullptr;          // recorded at the end of every write (main stream): the next precompute waits for it
    bool wdone_pending = false;
    // ---- ev_opstart: recorded on the main stream where a read_prepare_write STARTS (free there: nothing of the op has been enqueued yet); its gate wave waits for
    // it on the side stream.  A host that enqueues ops without waiting for them is ahead of the device: without this the gate wave could be
    // parked while the PREVIOUS op's 256-register chain launch is still being placed, and cost that launch a second round on one CU.
    // Only needed while a 256-register launch of an earlier op may still be waiting for its CUs: wide_unsynced = such a launch has been enqueued
    // and the host has not waited for the stream since (a host that waits for every op — the reference's calling pattern — never pays the record).
    hipEvent_t ev_opstart = nullptr;
    bool opstart_valid = false;
    bool wide_unsynced = false;
    // The second reason for the record: the side work reads the address's digits (coordinate_prepare_inv), and fheram_address_derive writes
    // them with a launch on the main stream that no host wait follows.  The gate wave is time-bounded, so it cannot be what orders that
    // read behind the launch: derive_unsynced = such a launch has been enqueued and the host has not waited for the stream since; the next
    // gated read_prepare_write then records ev_opstart behind it, whatever wide_unsynced says.
    bool derive_unsynced = false;
    // main_idle: the host has waited for the main stream (main_waited: fheram_sync, fheram_timer_end, the result export) and nothing with an
    // effect on memory has been enqueued on it since (main_enqueued: every operation's enqueue functions, the words' copy, the device-side
    // hand-overs, the stream waits, a derive launch; a bare event record — fheram_timer_begin — changes nothing a later launch could depend on).
    // The side stage of a write then has nothing to wait for on the main stream, and write_side_begin saves the fork event (a record and a
    // cross-stream wait in front of the write's first kernel).  Whoever enqueues on the main stream without waiting for it at its end clears the flag.
    bool main_idle = false;
    // ---- staging ----
    int32_t* h_pin[2] = {nullptr, nullptr};   // pinned host staging (hand-over of int64 host buffers), made on first use (pin_init)
    hipEvent_t ev_pin[2] = {nullptr, nullptr};
    // the two hand-overs ON the path (result of a read out, words of a write in) have staging of their own:
    //  h_res: pinned, device-visible; an export kernel widens the result into it as int64 in the ABI's layout (no DMA
    //         engine round trip, no host-side widening: the host copies it out, or reads it in place, fheram_result_map)
    //  h_w  : pinned; the host narrows the words into it and an asynchronous copy takes them to d_w — the call does not wait
    int64_t* h_res = nullptr;
    int64_t* d_h_res = nullptr;               // device address of h_res
    int32_t* h_w = nullptr;
    hipEvent_t ev_w = nullptr;
    bool w_busy = false;
    // ---- the write in flight ----
    bool side_begun = false;                          // write_side_begin has been enqueued for it
    bool trhi_in_C = false;                           // trace(ct_hi) of the local rows is in arena C (else A)
    bool tree_rotate_pending = false;                 // write_top left the tree's rotated copy of ct_lo to write_rows
    bool words_staged = false;
    // ---- profiling, and the error string ----
    int profile = 0;               // 1: every launch class bracketed by HIP events; 2: only the chain launches themselves (two events per launch: leaves back-to-back submission intact)
    std::map<std::string, ProfCls> prof;
    std::vector<hipEvent_t> ev_pool;   // events of collected launches, for reuse (get_event makes them through `res`)
    hipEvent_t t0 = nullptr, t1 = nullptr;
    std::string err;
};

struct fheram_addr {
    fheram_ctx* ctx;   // owner (identity check only after creation)
    int32_t* d_ggsw;   // [n_digits] std-form GGSW, int32
    int n_digits;
    int device;
    uint64_t id = next_addr_id();   // never reused (a freed address may be followed by another one at the same pointer)
    hipGraphExec_t graph[3] = {nullptr, nullptr, nullptr};   // captured launch sequences: read, read_prepare_write, write
    unsigned graph_sig[3] = {0, 0, 0};                       // context state the capture depended on (run_op)
    bool empty = false;                                      // fheram_address_alloc: buffers and no digits yet; read / write refuse it until fheram_address_derive has filled it
};

struct fheram_fheuint {
    fheram_ctx* ctx;
    int device, n_bits;
    int32_t* d_std;    // [n_bits] std-form GGSW (5 limbs, dnum 4), int32
    double* d_prep;    // the same, prepared
};

struct fheram_secret {
    fheram_ctx* ctx;
    int device;
    std::vector<int32_t> sk;   // N coefficients in {-1, 0, 1}
    double* d_hat;             // prepared (transform domain, 1/N folded in)
};

namespace {

int fail(fheram_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_err = msg;
    return code;
}
// Called wherever the host has just waited for the device: the sticky flag of the round-off monitor turns into a status.
int check_precision(fheram_ctx* c) {
    if (c->h_ro_flag && __atomic_load_n(c->h_ro_flag, __ATOMIC_RELAXED))
        return fail(c, FHERAM_ERR_PRECISION, "FP64 round-off of an inverse transform exceeded 3/8 (fheram_roundoff_max): the rounded integers are no longer trustworthy");
    return FHERAM_OK;
}
#define HIPCHK(c, call)                                                                     \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail((c), FHERAM_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

GlweRef ref(int32_t* p, long sy, long sx) { return GlweRef{p, sy, sx}; }

// the host has just waited for everything enqueued on the main stream / something is being enqueued on it (fheram_ctx: wide_unsynced, derive_unsynced, main_idle)
void main_waited(fheram_ctx* c) { c->wide_unsynced = c->derive_unsynced = false; c->main_idle = true; c->tail_wait.waited(); }
void main_enqueued(fheram_ctx* c) { c->main_idle = false; c->tail_wait.enqueued(); }

hipEvent_t get_event(fheram_ctx* c) {
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr; c->res.event(&e, true); return e;
}
struct ProfScope {
    fheram_ctx* c; ProfCls* cls = nullptr; hipEvent_t a = nullptr;
    // steps: ciphertext-operation rounds inside the launch (a chain kernel runs several): `launches` counts rounds,
    // so that ms / launches stays the time of ONE round over `blocks / launches` ciphertexts
    ProfScope(fheram_ctx* c_, const char* name, uint64_t blocks, int steps = 1) : c(c_) {
        if (!c->profile) return;
        if (c->profile == 2 && !strstr(name, "chain_launch")) return;
        cls = &c->prof[name];
        cls->launches += steps; cls->blocks += blocks * steps;
        a = get_event(c);
        hipEventRecord(a, c->cur);
    }
    ~ProfScope() {
        if (!cls) return;
        hipEvent_t b = get_event(c);
        hipEventRecord(b, c->cur);
        cls->pending.emplace_back(a, b);
    }
};
void prof_collect(fheram_ctx* c) {
    for (auto& kv : c->prof) {
        for (auto& pr : kv.second.pending) {
            hipEventSynchronize(pr.second);
            float ms = 0.f;
            hipEventElapsedTime(&ms, pr.first, pr.second);
            kv.second.ms += ms;
            c->ev_pool.push_back(pr.first); c->ev_pool.push_back(pr.second);
        }
        kv.second.pending.clear();
    }
}

// get_base_2d (base.rs:84-108): the digit plan of a RAM of max_addr words over the parameters' DECOMP_N, one vector of digit widths per coordinate
std::vector<std::vector<int>> base_2d(uint64_t max_addr, const fheram_params& p) {
    std::vector<std::vector<int>> plan;
    uint32_t x = (uint32_t)(max_addr - 1), bits = 0;
    while (x) { bits++; x >>= 1; }
    while (bits != 0) {
        std::vector<int> v;
        for (uint32_t i = 0; i < p.n_decomp; i++) {
            const uint32_t b = p.decomp_n[i];
            if (b <= bits) { v.push_back((int)b); bits -= b; }
            else { if (bits != 0) { v.push_back((int)bits); bits = 0; } break; }
        }
        plan.push_back(v);
    }
    return plan;
}
int ilog2_ceil(size_t x) { int k = 0; while (((size_t)1 << k) < x) k++; return k; }
int galois_mod(int64_t g) { const int64_t m = 2 * N; return (int)(((g % m) + m) % m); }
int galois_inv_mod(int g) {   // g odd; g^(N-1) = g^-1 mod 2N
    int64_t r = 1, b = g, e = N - 1, m = 2 * N;
    while (e) { if (e & 1) r = r * b % m; b = b * b % m; e >>= 1; }
    return (int)r;
}
int64_t galois_element(int i) {   // GLWE::trace_galois_elements (keys.rs:39,158)
    if (i == 0) return -1;
    int64_t g = 5, e = (int64_t)1 << (i - 1), r = 1, m = 2 * N;
    while (e) { if (e & 1) r = r * g % m; g = g * g % m; e >>= 1; }
    return r;
}

// ---- narrowing / widening between the int64 ABI layout and the int32 device layout ---------
bool narrow(const int64_t* src, int32_t* dst, size_t n) {
    int64_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        const int64_t v = src[i];
        bad |= (v > 65536) | (v < -65536);
        dst[i] = (int32_t)v;
    }
    return bad == 0;
}
void widen(const int32_t* src, int64_t* dst, size_t n) { for (size_t i = 0; i < n; i++) dst[i] = src[i]; }

// The hand-over goes through two pinned staging buffers of PIN_CHUNK elements: the narrowing / widening
// of one chunk overlaps the DMA of the other, and the DMA itself runs at the pinned-memory rate (a
// pageable copy is staged by the runtime a second time).  Both calls return when the data has arrived.
constexpr size_t PIN_CHUNK = (size_t)1 << 21;   // int32 elements per staging buffer (8 MiB)
int pin_init(fheram_ctx* c) {
    if (c->h_pin[0]) return FHERAM_OK;
    for (int b = 0; b < 2; b++) {
        HIPCHK(c, c->res.host(&c->h_pin[b], PIN_CHUNK * sizeof(int32_t), hipHostMallocDefault));
        HIPCHK(c, c->res.event(&c->ev_pin[b]));
    }
    return FHERAM_OK;
}
int upload_i64(fheram_ctx* c, int32_t* dst, const int64_t* src, size_t n) {
    int rc = pin_init(c);
    if (rc != FHERAM_OK) return rc;
    bool ok = true;
    int k = 0;
    for (size_t off = 0; off < n && ok; off += PIN_CHUNK, k++) {
        const int b = k & 1;
        const size_t m = std::min(PIN_CHUNK, n - off);
        if (k >= 2) HIPCHK(c, hipEventSynchronize(c->ev_pin[b]));   // the copy that last used this buffer is done
        ok = narrow(src + off, c->h_pin[b], m);
        if (!ok) break;
        HIPCHK(c, hipMemcpyAsync(dst + off, c->h_pin[b], m * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_pin[b], c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!ok) return fail(c, FHERAM_ERR_RANGE, "limb out of the normalised range [-2^16, 2^16]");
    return FHERAM_OK;
}
int download_i64(fheram_ctx* c, int64_t* dst, const int32_t* src, size_t n) {
    int rc = pin_init(c);
    if (rc != FHERAM_OK) return rc;
    const size_t n_chunks = (n + PIN_CHUNK - 1) / PIN_CHUNK;
    for (size_t k = 0; k <= n_chunks; k++) {
        if (k < n_chunks) {   // request chunk k
            const size_t off = k * PIN_CHUNK, m = std::min(PIN_CHUNK, n - off);
            HIPCHK(c, hipMemcpyAsync(c->h_pin[k & 1], src + off, m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipEventRecord(c->ev_pin[k & 1], c->stream));
        }
        if (k > 0) {          // widen chunk k - 1 while chunk k is in flight
            const size_t off = (k - 1) * PIN_CHUNK, m = std::min(PIN_CHUNK, n - off);
            HIPCHK(c, hipEventSynchronize(c->ev_pin[(k - 1) & 1]));
            widen(c->h_pin[(k - 1) & 1], dst + off, m);
        }
    }
    return FHERAM_OK;
}
// The words of a write, n_ct ciphertexts, on their way to d_w: narrowed into the pinned buffer h_w and copied asynchronously — the call
// does not wait for the copy (the kernels that read d_w are ordered behind it on the stream; h_w is reused only after its event).
int stage_words(fheram_ctx* c, int32_t* d_w, const int64_t* w, int n_ct) {
    if (c->w_busy) { HIPCHK(c, hipEventSynchronize(c->ev_w)); c->w_busy = false; }
    const size_t n = (size_t)n_ct * fheram_ctx::GLWE;
    if (!narrow(w, c->h_w, n)) return fail(c, FHERAM_ERR_RANGE, "limb out of the normalised range [-2^16, 2^16]");
    main_enqueued(c);
    HIPCHK(c, hipMemcpyAsync(d_w, c->h_w, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_w, c->stream));
    c->w_busy = true;
    return FHERAM_OK;
}

}  // namespace
