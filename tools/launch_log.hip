// Launch log of the host code's chain dispatch, on the CPU: nothing is launched and no GPU is opened.
//
// hipLaunchKernelGGL is redefined as a recorder of (kernel, grid, workgroup, LDS bytes, stream side, argument bytes); with fake,
// distinct addresses in the context's buffer fields the program calls trace_steps, ep_chain, pack_levels, the row-chain and tail launchers and the predicates path.hpp
// derives from the same decision (Opnds::row_fuse for a context, a batch and a bank range; third_arena_needed; read_top's fuse_ep /
// gated) over a sweep of configurations, chain lengths, grids and buffer layouts.  Two trees dispatch alike exactly when their logs are
// equal, so a change to a launch form is one `diff` away from its evidence:
//
//   hipcc -std=c++17 -O1 --offload-arch=gfx950 -ftrivial-auto-var-init=zero -Wno-unused-variable -Wno-unused-value -Wl,--unresolved-symbols=ignore-all -I fhe-ram_amd/csrc -I tools -o launch_log tools/launch_log.hip
//   ./launch_log > chain_log.txt                           one digest line per configuration (FNV-1a over its launch lines); the committed
//                                                          profiles/chain_form_launch_log.txt is the tree's of DESIGN.md 10.2, later ones are recorded by hash (10.5)
//   ./launch_log 17                                        every launch line of configuration 17
//
// -ftrivial-auto-var-init=zero makes the padding of the argument structs part of a reproducible digest.  The include path names the
// csrc/ to log; launch_log_shim.hpp (tools/ for this tree) reaches what has no name of its own there.
// Trace chains are logged for 0 .. LOGN steps (the context has LOGN trace keys), product chains and the predicates for 0 .. CHAIN_MAX + 1.
//
// Second mode, the SEQUENCES themselves (path.hpp read_impl and the write triple) for a context, a batch, ranges of a bank's members and
// read lists and read_prepare_write / write lists of a bank of three; behind the configurations, in full: the REFUSALS of the bank's
// checks (code, message and the mid re-arm count, one line per bad argument) and the RESERVE log of the dense buffer sets (hipMalloc and
// its kin are recorders too: every allocation, free and stream wait of a sequence of reserves, and what the set holds afterwards):
//
//   ./launch_log path > path_log.txt                       one digest line per configuration, then the refusals and the reserves (profiles/ram_view_path_log.txt: the tree's
//                                                          of DESIGN.md 10.4; profiles/member_set_path_log.txt: with the write lists, the refusals and the reserves, 10.7)
//   ./launch_log path 17                                   every line of configuration 17
//
// Every buffer is a fake arena 4 GiB from the next, so an argument that points into one shows as a<arena>+<byte offset> behind the launch's
// digest, events show as record / wait lines, and after every operation the log holds each RAM's state, the flags of the write in flight and
// the context's buffer fields and word count: a range's pointer arithmetic, and anything an operation leaves behind in the context, is in
// the log.  What differs between trees — how a bank range is presented to the sequences, where the per-RAM state lives — is in the shim.
// bank.hpp names entry points of fheram.hip that this program never calls: link with -Wl,--unresolved-symbols=ignore-all.
// Fourth mode, `./launch_log onerow`: the operations that keep last outputs, stage host words and read one-row RAMs —
// select, select_lanes, the register file, the tables, both mixes, peek and poke — through their entry points, on a bank of two at word
// sizes 2 and 13: every launch, copy and event, and after every operation each kind's last-outputs record and what select_source
// gives for it (one digest line per configuration; `./launch_log onerow <id>` prints one in full); then those operations' refusals and the reserve log of their buffer sets, the three self-test failing allocations at every
// nth included.  The launchers of the other translation units are recorders here; pinned allocations are real memory at fixed addresses
// (profiles/one_row_kinds_log.txt).
// Third mode, `./launch_log config`: the switches IN EFFECT (ctx.hpp config_in_effect) for a list of requested configurations, one line per
// input, both sides as departures from the built-in defaults D (profiles/ctx_config_in_effect.txt: the tree's of DESIGN.md 10.6).
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace ll {
bool verbose = false, path_mode = false;
uint64_t digest = 0, lines = 0;
hipStream_t main_stream = nullptr;
uint64_t fnv(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}
void line(const std::string& s) {
    digest = fnv(fnv(digest, s.data(), s.size()), "\n", 1);
    lines++;
    if (verbose) std::puts(s.c_str());
}
// "NAME = value" of a template parameter in __PRETTY_FUNCTION__; a generic lambda's `auto sk` shows as "sk:auto = std::integral_constant<int, value>"
bool param(const std::string& site, const std::string& name, std::string& val) {
    for (size_t at = 0; (at = site.find(name + " = ", at)) != std::string::npos; at++) {
        if (at > 0 && (std::isalnum((unsigned char)site[at - 1]) || site[at - 1] == '_')) continue;
        size_t b = at + name.size() + 3, e = b;
        while (e < site.size() && (std::isalnum((unsigned char)site[e]) || site[e] == '_')) e++;
        val = site.substr(b, e - b);
        return true;
    }
    std::string lower = name;
    for (char& ch : lower) ch = (char)std::tolower((unsigned char)ch);
    const std::string key = lower + ":auto = std::integral_constant<";
    const size_t at = site.find(key);
    if (at == std::string::npos) return false;
    size_t b = site.find(", ", at) + 2, e = b;
    while (e < site.size() && site[e] != '>') e++;
    val = site.substr(b, e - b);
    return true;
}
// the kernel as written at the launch site, with the template parameters of the enclosing launcher filled in
std::string kernel_name(const char* text, const char* site_) {
    const std::string t = text, site = site_;
    std::string out;
    for (size_t i = 0; i < t.size();) {
        if (std::isalpha((unsigned char)t[i]) || t[i] == '_') {
            size_t e = i;
            while (e < t.size() && (std::isalnum((unsigned char)t[e]) || t[e] == '_')) e++;
            std::string id = t.substr(i, e - i), val;
            out += (id.find("k_") != 0 && param(site, id, val)) ? val : id;
            i = e;
        } else {
            if (t[i] != ' ' && t[i] != '(' && t[i] != ')') out += t[i];
            i++;
        }
    }
    return out;
}
// a fake device address (arena k of fake<>() below: k + 1 in the upper half) as a<k>+<byte offset>; anything else: empty
std::string arena_of(uint64_t v) {
    if (v < 0x100000000ull || v >= 0x10000000000ull) return "";
    char buf[48];
    std::snprintf(buf, sizeof buf, "a%u+%#x", (unsigned)(v >> 32) - 1, (unsigned)v);
    return buf;
}
void arenas_in(std::string& out, const void* p, size_t n) {   // the 8-byte words of an argument that hold such an address
    for (size_t i = 0; i + 8 <= n; i += 8) {
        uint64_t v;
        std::memcpy(&v, static_cast<const char*>(p) + i, 8);
        const std::string a = arena_of(v);
        if (!a.empty()) out += " " + a;
    }
}
template <typename... A>
void record(const char* kernel, const char* site, dim3 g, dim3 b, size_t lds, hipStream_t s, const A&... a) {
    uint64_t h = 0xcbf29ce484222325ull;
    size_t bytes = 0;
    ((h = fnv(h, &a, sizeof(a)), bytes += sizeof(a)), ...);
    char buf[512];
    std::snprintf(buf, sizeof buf, "  %s grid=(%u,%u,%u) wg=%u lds=%zu %s args=%zuB:%016" PRIx64, kernel_name(kernel, site).c_str(), g.x, g.y, g.z, b.x, lds,
                  s == main_stream ? "main" : "side", bytes, h);
    std::string l = buf;
    if (path_mode) (arenas_in(l, &a, sizeof(a)), ...);
    line(l);
}
// the reserve log: the allocations, frees and stream waits (these in reserve_mode only) of one call; fail_nth: the fail_nth-th next allocation reports an exhausted device
bool reserve_mode = false;
int fail_nth = 0;
unsigned n_alloc = 0;
// (one line per call of the reserve log: its events in order, a run of equal events as "<event> x<count>")
std::string call_events, last_event;
unsigned last_count = 0;
void flush_event() {
    if (last_count) call_events += (call_events.empty() ? "" : ", ") + last_event + (last_count > 1 ? " x" + std::to_string(last_count) : "");
    last_count = 0;
}
void call_event(const std::string& e) {
    if (last_count && e == last_event) { last_count++; return; }
    flush_event();
    last_event = e; last_count = 1;
}
std::string take_events() { flush_event(); std::string e = call_events.empty() ? "nothing" : call_events; call_events.clear(); return e; }
hipError_t alloc(void** p, size_t bytes, const char* kind) {
    if (fail_nth > 0 && --fail_nth == 0) { call_event(std::string(kind) + " " + std::to_string(bytes) + " -> out of memory"); return hipErrorOutOfMemory; }
    *p = reinterpret_cast<void*>((uintptr_t)0x100000000ull * (uintptr_t)(129 + n_alloc++ % 100));
    call_event(std::string(kind) + " " + std::to_string(bytes));
    return hipSuccess;
}
hipError_t release(const char* what) { call_event(what); return hipSuccess; }
hipError_t sync(hipStream_t s) {
    if (reserve_mode) call_event(s == main_stream ? "wait main" : "wait side");
    return hipSuccess;
}
hipError_t event(const char* what, const void* ev, hipStream_t s) {
    if (path_mode) line(std::string("  ") + what + " " + arena_of((uint64_t)(uintptr_t)ev) + (s == main_stream ? " main" : " side"));
    return hipSuccess;
}
// onerow mode: pinned allocations have real, zeroed memory behind them (narrow and result_export touch it), allocation k at a fixed
// address, so that the argument digests are reproducible; it shows as p<k>+<byte offset>.  Events are fake addresses of their own
// (a230 ..), created, waited for and destroyed in the reserve log; copies are lines of the sequence.
bool onerow_mode = false;
constexpr uintptr_t PINNED_BASE = 0x7d0000000000ull, PINNED_STEP = 0x10000000ull;
unsigned n_pinned = 0, n_events = 0;
hipError_t alloc_pinned(void** p, size_t bytes) {
    if (!onerow_mode) return alloc(p, bytes, "alloc pinned");
    if (fail_nth > 0 && --fail_nth == 0) { call_event("alloc pinned " + std::to_string(bytes) + " -> out of memory"); return hipErrorOutOfMemory; }
    void* want = reinterpret_cast<void*>(PINNED_BASE + PINNED_STEP * n_pinned++);
    if (bytes > PINNED_STEP || mmap(want, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_FIXED_NOREPLACE, -1, 0) != want) { std::perror("mmap (pinned)"); std::exit(1); }
    *p = want;
    call_event("alloc pinned " + std::to_string(bytes));
    return hipSuccess;
}
std::string ptr_name(const void* p) {
    const uintptr_t v = (uintptr_t)p;
    if (!p) return "0";
    if (v >= PINNED_BASE && v < PINNED_BASE + PINNED_STEP * n_pinned) {
        char buf[48];
        std::snprintf(buf, sizeof buf, "p%u+%#x", (unsigned)((v - PINNED_BASE) / PINNED_STEP), (unsigned)((v - PINNED_BASE) % PINNED_STEP));
        return buf;
    }
    const std::string a = arena_of(v);
    return a.empty() ? "host" : a;
}
hipError_t copy(const void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const char* how, hipStream_t s) {
    const char* k = kind == hipMemcpyHostToDevice ? "h2d" : kind == hipMemcpyDeviceToHost ? "d2h" : kind == hipMemcpyDeviceToDevice ? "d2d" : "copy";
    const std::string l = std::string(how) + " " + k + " " + ptr_name(dst) + " <- " + ptr_name(src) + " " + std::to_string(bytes) + "B" + (s == main_stream ? " main" : " side");
    if (path_mode) line("  " + l);
    if (reserve_mode) call_event(l);
    return hipSuccess;
}
hipError_t event_create(hipEvent_t* e) {
    *e =reinterpret_cast<hipEvent_t>((uintptr_t)0x100000000ull * (uintptr_t)(231 + n_events++ % 24));
    call_event("event");
    return hipSuccess;
}
hipError_t event_sync(hipEvent_t e) {
    if (path_mode) line("  sync " + arena_of((uint64_t)(uintptr_t)e));
    if (reserve_mode) call_event("wait event");
    return hipSuccess;
}
}  // namespace ll

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) ll::record(#kernel, __PRETTY_FUNCTION__, grid, block, lds, stream, __VA_ARGS__)
// no event is created, recorded or waited for, no stream waited for (ProfScope under `profile`; the sequences of path mode, where record and wait are logged)
#define hipEventCreate(e) (*(e) = nullptr, hipSuccess)
#define hipEventRecord(e, s) ll::event("record", e, s)
#define hipStreamWaitEvent(s, e, flags) ll::event("wait", e, s)
#define hipStreamSynchronize(s) ll::sync(s)
#define hipGetLastError() hipSuccess
#define hipSetDevice(d) ((void)(d), hipSuccess)
// nothing is allocated: a fake address back, and a line in the reserve log
#define hipMalloc(p, bytes) ll::alloc((void**)(p), bytes, "alloc")
#define hipHostMalloc(p, bytes, flags) ll::alloc_pinned((void**)(p), bytes)
#define hipHostGetDevicePointer(d, h, flags) (*(d) = (h), hipSuccess)
#define hipFree(p) ll::release("free")
#define hipHostFree(p) ll::release("free pinned")
// no copy is made; events with flags (the host stages') are fake addresses (onerow mode)
#define hipMemcpyAsync(dst, src, bytes, kind, s) ll::copy(dst, src, bytes, kind, "copy", s)
#define hipMemcpy(dst, src, bytes, kind) ll::copy(dst, src, bytes, kind, "copy (blocking)", ll::main_stream)
#define hipEventCreateWithFlags(e, flags) ll::event_create(e)
#define hipEventSynchronize(e) ll::event_sync(e)
#define hipEventDestroy(e) ll::release("event destroy")

#include "mix.hpp"         // (bank.hpp, select.hpp, regs.hpp and table.hpp with it)
#include "public_io.hpp"
#include <launch_log_shim.hpp>   // (angle brackets: from the include path, not from beside this file)

// the launchers of the other translation units (mapped_chains.hip: the write lists' row chains; select_pack.hip, select_lanes.hip, regs.hip,
// table.hip, mix.hip, public_io.hip, cmux_chain.hip): here they are recorders like every other launch
namespace fk {
void read_chain_m_launch(int sk, dim3 grid, hipStream_t stream, const RowChainTableArgs& ra) { ll::record(("k_read_chain_m<" + std::to_string(sk) + ">").c_str(), "", grid, dim3(256), 0, stream, ra); }
void write_chain_m_launch(int sk, dim3 grid, hipStream_t stream, const RowChainTableArgs& ra) { ll::record(("k_write_chain_m<" + std::to_string(sk) + ">").c_str(), "", grid, dim3(256), 0, stream, ra); }
void select_pack_launch(dim3 grid, hipStream_t stream, const SelectPackArgs& sa) { ll::record("k_select_pack", "", grid, dim3(256), 0, stream, sa); }
void select_lanes_launch(int n_ct, hipStream_t stream, const SelectLanesArgs& sa) { ll::record("k_select_pack_lanes", "", dim3(1, n_ct, SELECT_LANES_SLICES), dim3(256), 0, stream, sa); }
void regs_fan_launch(int n_ct, hipStream_t stream, const RegsFanArgs& fa) { ll::record("k_regs_fan", "", dim3(1, n_ct, REGS_SLICES), dim3(256), 0, stream, fa); }
void regs_merge_launch(int ws, hipStream_t stream, const RegsMergeArgs& ma) { ll::record("k_regs_merge", "", dim3(1, ws, REGS_SLICES), dim3(256), 0, stream, ma); }
void table_fan_launch(int n_ct, hipStream_t stream, const TableFanArgs& fa) { ll::record("k_table_fan", "", dim3(1, n_ct, TABLE_SLICES), dim3(256), 0, stream, fa); }
void table_encode_launch(int ws, hipStream_t stream, const TableEncodeArgs& ea) { ll::record("k_table_encode", "", dim3(1, ws, TABLE_SLICES), dim3(256), 0, stream, ea); }
hipError_t mix_register() { ll::call_event("mix_register"); return hipSuccess; }
void trace_tail_x_launch(int sk, hipStream_t stream, const TailMixArgs& ta) { ll::record(("k_trace_tail_x<" + std::to_string(sk) + ">").c_str(), "", dim3(TAIL_GROUPS * 2 * sk * 3), dim3(256), 0, stream, ta); }
void read_chain_x_launch(int sk, int n_ct, hipStream_t stream, const RowChainMixArgs& ra) { ll::record(("k_read_chain_x<" + std::to_string(sk) + ">").c_str(), "", dim3(1, n_ct), dim3(256), 0, stream, ra); }
void mix_scatter_launch(int ws, hipStream_t stream, const MixScatterArgs& sa) { ll::record("k_mix_scatter", "", dim3(sa.n, ws, MIX_SCATTER_SLICES), dim3(256), 0, stream, sa); }
void rows_plain_launch(int n_rows, hipStream_t stream, const RowsPlainArgs& ra) { ll::record("k_rows_plain", "", dim3(n_rows, ra.ws, PUB_SLICES), dim3(256), 0, stream, ra); }
void peek_gather_launch(int n_ct, hipStream_t stream, const PeekGatherArgs& ga) { ll::record("k_peek_gather", "", dim3(1, n_ct, PUB_SLICES), dim3(256), 0, stream, ga); }
void poke_merge_launch(int n_touched, int ws, hipStream_t stream, const PokeMergeArgs& ma) { ll::record("k_poke_merge", "", dim3(n_touched, ws, PUB_SLICES), dim3(256), 0, stream, ma); }
void cmux_chain_launch(dim3 grid, hipStream_t stream, const CmuxChainArgs& ca) { ll::record("k_cmux_chain", "", grid, dim3(256), 0, stream, ca); }
}  // namespace fk

namespace {

template <typename P> P fake(int k) { return reinterpret_cast<P>((uintptr_t)0x100000000ull * (uintptr_t)(k + 1)); }
int32_t* arena(int k) { return fake<int32_t*>(32 + k); }

struct Setting { const char* name; void (*apply)(fheram_ctx*); };
const Setting SETTINGS[] = {
    {"default", [](fheram_ctx*) {}},
    {"nco=1", [](fheram_ctx* c) { c->cfg.nco = 1; }},
    {"nco=2", [](fheram_ctx* c) { c->cfg.nco = 2; }},
    {"limb_split=0", [](fheram_ctx* c) { c->cfg.limb_split = 0; }},
    {"fine_split=0", [](fheram_ctx* c) { c->cfg.fine_split = 0; }},
    {"tail=0", [](fheram_ctx* c) { c->cfg.tail = 0; }},
    {"tail_test=1", [](fheram_ctx* c) { c->cfg.tail_test = 1; }},
    {"tail_test=2", [](fheram_ctx* c) { c->cfg.tail_test = 2; }},
    {"tail_ep=0", [](fheram_ctx* c) { c->cfg.tail_ep = 0; }},
    {"mid=0", [](fheram_ctx* c) { c->cfg.mid = 0; }},
    {"mid=1", [](fheram_ctx* c) { c->cfg.mid = 1; }},
    {"mid_test=1", [](fheram_ctx* c) { c->cfg.mid_test = 1; }},
    {"chain=0", [](fheram_ctx* c) { c->cfg.chain = 0; }},
    {"chain_y=0", [](fheram_ctx* c) { c->cfg.chain_y = 0; }},
    {"fuse=0", [](fheram_ctx* c) { c->cfg.fuse = 0; }},
    {"pair_z=0", [](fheram_ctx* c) { c->cfg.pair_z = 0; }},
    {"safe", [](fheram_ctx* c) { c->cfg.safe = 1; c->cfg.tail = 0; c->cfg.tail_test = 0; c->cfg.mid = 0; c->cfg.mid_test = 0; }},
    {"wide", [](fheram_ctx* c) { c->wide = true; }},
    // the pairs the test suite forces
    {"limb_split=0,nco=1", [](fheram_ctx* c) { c->cfg.limb_split = 0; c->cfg.nco = 1; }},
    {"limb_split=0,nco=2", [](fheram_ctx* c) { c->cfg.limb_split = 0; c->cfg.nco = 2; }},
    {"limb_split=0,nco=2,wide", [](fheram_ctx* c) { c->cfg.limb_split = 0; c->cfg.nco = 2; c->wide = true; }},
    {"limb_split=0,nco=2,chain=0", [](fheram_ctx* c) { c->cfg.limb_split = 0; c->cfg.nco = 2; c->cfg.chain = 0; }},
    {"limb_split=0,nco=2,chain_y=0", [](fheram_ctx* c) { c->cfg.limb_split = 0; c->cfg.nco = 2; c->cfg.chain_y = 0; }},
    {"limb_split=0,nco=2,chain_y=0,wide", [](fheram_ctx* c) { c->cfg.limb_split = 0; c->cfg.nco = 2; c->cfg.chain_y = 0; c->wide = true; }},
    {"limb_split=0,nco=2,fuse=0,pair_z=0", [](fheram_ctx* c) { c->cfg.limb_split = 0; c->cfg.nco = 2; c->cfg.fuse = 0; c->cfg.pair_z = 0; }},
    {"chain_y=0,fuse=0,nco=2,limb_split=0", [](fheram_ctx* c) { c->cfg.chain_y = 0; c->cfg.fuse = 0; c->cfg.nco = 2; c->cfg.limb_split = 0; }},
    {"mid=0,tail=0", [](fheram_ctx* c) { c->cfg.mid = 0; c->cfg.tail = 0; }},
    {"tail_ep=0,tail_test=1", [](fheram_ctx* c) { c->cfg.tail_ep = 0; c->cfg.tail_test = 1; }},
    {"nco=2,mid=0", [](fheram_ctx* c) { c->cfg.nco = 2; c->cfg.mid = 0; }},
    {"nco=2,fine_split=0", [](fheram_ctx* c) { c->cfg.nco = 2; c->cfg.fine_split = 0; }},
};
const int CUS[] = {64, 128, 256, 304};
const int GX[] = {1, 2, 3, 4, 8, 9, 16, 17, 32, 64, 65, 128, 256, 512, 2048};
const int GY[] = {1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 32, 64};

// a context with default member initialisers only, fake device addresses and real (zeroed, fixed-address) host words
fheram_ctx* make_ctx(unsigned* host_words) {
    fheram_ctx* c = new fheram_ctx();
    c->stream = fake<hipStream_t>(0); c->stream2 = fake<hipStream_t>(1);
    ll::main_stream = c->stream;
    c->d_tw = fake<double*>(2); c->d_atk = fake<double*>(3); c->d_big = fake<double*>(4); c->d_big2 = fake<double*>(5);
    c->d_tail_sync = fake<unsigned*>(6);
    for (int s = 0; s < 2; s++) { c->d_mid_sync[s] = fake<unsigned*>(7 + s); c->d_mid_big[s] = fake<double*>(9 + s); c->d_mid_y[s] = fake<double*>(11 + s); }
    c->d_prep = fake<double*>(13);
    c->h_tail_fb = host_words; c->h_mid_fb = host_words + 64;
    for (int i = 0; i < LOGN; i++) c->gal[i] = galois_element(i);
    c->n2 = 2; c->ws = 1; c->rows = c->rows_glob = 1;
    c->base2d = {{1, 1, 1}, {1, 1, 1}};
    return c;
}
// what a launch advances: every case starts from the same counters
void rewind(fheram_ctx* c, const fheram_ctx* as) {
    c->cfg.tail = as->cfg.tail; c->tail_seq = 0; c->tail_launches = c->tail_launch_mark = 0; c->tail_fb_mark = 0;
    c->cfg.mid = as->cfg.mid; c->mid_seq = 0; c->mid_launches = c->mid_launch_mark = 0; c->mid_fb_mark = 0; c->mid_bad_windows = c->mid_saved = 0;
    c->mid_window_cts = c->mid_disabled_count = 0; c->wide_unsynced = false;
    c->prof.clear();
}
void head(const char* what, int n, int gx, int gy, int v) {
    char buf[128];
    std::snprintf(buf, sizeof buf, "%s n=%d grid=(%d,%d) variant=%d", what, n, gx, gy, v);
    ll::line(buf);
}
void tail_line(const char* what, long v) {
    char buf[128];
    std::snprintf(buf, sizeof buf, "  -> %s %ld", what, v);
    ll::line(buf);
}

uint64_t cases = 0;
void run_config(fheram_ctx* c) {
    const fheram_ctx* as = nullptr;
    fheram_ctx keep_cfg = *c;
    as = &keep_cfg;
    const long sy = (long)2048 * (long)fheram_ctx::GLWE, sx = (long)fheram_ctx::GLWE;
    int32_t *S = arena(0), *A = arena(1), *B = arena(2), *C = arena(3), *D = arena(4);
    for (int n = 0; n <= CHAIN_MAX + 1; n++)
    for (int gx : GX)
    for (int gy : GY) {
        // trace chains: out of place, in place, scratch = source; each unrotated and rotated
        if (n <= LOGN) for (int v = 0; v < 6; v++) {
            rewind(c, as); cases++;
            head("trace_steps", n, gx, gy, v);
            const GlweRef src = ref(S, sy, sx), dst = ref(v % 3 == 1 ? S : A, sy, sx), tmp = ref(v % 3 == 2 ? S : B, sy, sx);
            trace_steps(c, src, dst, tmp, 0, n, gx, gy, v >= 3 ? 2 : 0, v >= 3 ? 1 : 0);
        }
        // a later start: the keys a chain names
        if (n >= 1 && n < LOGN && gx == 8) { rewind(c, as); cases++; head("trace_steps_from_1", n, gx, gy, 0); trace_steps(c, ref(S, sy, sx), ref(A, sy, sx), ref(B, sy, sx), 1, n + 1, gx, gy); }
        for (int v = 0; v < 3; v++) {
            rewind(c, as); cases++;
            head("ep_chain", n, gx, gy, v);
            ep_chain(c, ref(S, sy, sx), ref(v == 1 ? S : A, sy, sx), ref(v == 2 ? S : B, sy, sx), c->d_prep, n, gx, gy);
        }
        // the packer: leaves outside / inside the ping-pong arenas, third (and fourth) arena or not, keep_alone
        if (n <= LOGN - ilog2_ceil((size_t)gx)) for (int v = 0; v < 6; v++) {
            rewind(c, as); cases++;
            head("pack_levels", n, gx, gy, v);
            int32_t* src = (v & 1) ? A : S;
            const bool third = v & 2, keep = v >= 4;
            if (keep && src == A) src = B;   // (variant 5: leaves in the second arena)
            const int32_t* packed = pack_levels(c, src, A, B, sy, sx, (size_t)gx, gy, n, LOGN - ilog2_ceil((size_t)gx), keep && src == S, third || keep ? C : nullptr, third || keep ? D : nullptr);
            tail_line("packed in arena", (long)((uintptr_t)packed >> 32) - 33);
        }
        // the launchers path.hpp calls directly (which instantiation they name): the row chains and the tail with products, without and with an operand table
        if (n >= 1 && n <= TAIL_EP_MAX && (gx == 1 || gx == 64) && (gy == 4 || gy == 8)) for (int v = 0; v < 2; v++) {
            rewind(c, as); cases++;
            head("row_chains", n, gx, gy, v);
            const OpndTable t = v ? shim_table(gy) : OpndTable{};
            const GlweRef rows = ref(S, sy, sx), a = ref(A, sy, sx), part = ref(D, sx, 0), out = ref(C, sx, 0);
            launch_read_chain(c, rows, nullptr, a, c->d_prep, n, LOGN - ilog2_ceil((size_t)gx), gx, gy, t);
            launch_read_chain(c, rows, &rows, a, c->d_prep, n, LOGN - ilog2_ceil((size_t)gx), gx, gy, t);
            launch_write_chain(c, part, 2, 1, rows, a, c->d_prep, n, LOGN, gx, gy, t);
            if (gx == 1) {
                GlweRef tb[2];
                if (chain_bufs(LOGN, part, out, ref(B, sx, 0), tb)) launch_trace_tail(c, part, tb, 0, LOGN, 1, gy, c->d_prep, n, ref(A, sx, 0), v == 1, t);
            }
        }
        // the predicates path.hpp derives
        rewind(c, as); cases++;
        head("predicates", n, gx, gy, 0);
        long bits = 0;
        for (int n_tr = 0; n_tr <= CHAIN_MAX + 1; n_tr++) {
            const Opnds ctx = shim_opnds(c, 1, gy, true), batch = shim_opnds(c, 2, (gy + 1) / 2, false), bank = shim_opnds(c, 2, (gy + 1) / 2, true);
            bits = bits * 8 + (ctx.row_fuse(n, n_tr, gx) ? 1 : 0) + (batch.row_fuse(n, n_tr, gx) ? 2 : 0) + (bank.row_fuse(n, n_tr, gx) ? 4 : 0);
        }
        tail_line("row_fuse (ctx, batch, bank) x n_tr", bits);
        c->rows = (size_t)gx; c->ws = 1; c->base2d[0].assign((size_t)std::max(n, 1), 1);
        bits = 0;
        for (int lg = 0; lg <= LOGN; lg++) { c->rows_glob = (size_t)1 << lg; bits = bits * 2 + (shim_needs_third(c, gy) ? 1 : 0); }
        tail_line("third_arena_needed x log2(rows)", bits);
        tail_line("read_top tail (fuse_ep, gated)", shim_tail_top(c, gx * gy) ? 1 : 0);
        c->rows = c->rows_glob = 1; c->base2d[0].assign(3, 1);
    }
}

// ---- path mode: the sequences on a context, a batch and ranges of a bank's members ---------------------------------------------------
// the switch settings the bank suite forces (tests/test_gpu_bank.py FORMS, as fheram_ctx_create_cfg derives them)
const Setting PATH_SETTINGS[] = {
    {"default", [](fheram_ctx*) {}},
    {"tail=0", [](fheram_ctx* c) { c->cfg.tail = 0; }},
    {"tail_ep=0", [](fheram_ctx* c) { c->cfg.tail_ep = 0; }},
    {"mid=0", [](fheram_ctx* c) { c->cfg.mid = 0; }},
    {"fuse=0", [](fheram_ctx* c) { c->cfg.fuse = 0; }},
    {"chain_y=0", [](fheram_ctx* c) { c->cfg.chain_y = 0; }},
    {"memo=0", [](fheram_ctx* c) { c->cfg.memo = 0; c->cfg.pre_inv = 0; }},
    {"pre_inv=0", [](fheram_ctx* c) { c->cfg.pre_inv = 0; }},
    {"pre_inv=2", [](fheram_ctx* c) { c->cfg.pre_inv = 2; }},
    {"safe", [](fheram_ctx* c) { c->cfg.safe = 1; c->cfg.tail = 0; c->cfg.tail_test = 0; c->cfg.mid = 0; c->cfg.mid_test = 0; c->cfg.pre_inv = 2; c->cfg.monitor = 2; }},
};
const int PATH_LOG_MAX_ADDR[] = {12, 13, 14, 16, 18};

// the buffers indexed by ciphertext: arena(i) for field i; the batch's: arena(16 + i); a read list's: fake(64 + i)
struct Field { const char* name; int32_t* fheram_ctx::*p; };
const Field FIELDS[] = {{"data", &fheram_ctx::d_data}, {"scrA", &fheram_ctx::d_scrA}, {"scrB", &fheram_ctx::d_scrB}, {"scrC", &fheram_ctx::d_scrC},
                        {"scrD", &fheram_ctx::d_scrD}, {"tree", &fheram_ctx::d_tree}, {"res", &fheram_ctx::d_res}, {"tmp", &fheram_ctx::d_tmp},
                        {"tmp2", &fheram_ctx::d_tmp2}, {"w", &fheram_ctx::d_w}, {"part", &fheram_ctx::d_part}, {"trtop", &fheram_ctx::d_trtop}};
const char* const READS_FIELDS[] = {"A", "B", "C", "res", "tmp", "tmp2"};   // (the shim's shim_batch_field / shim_list_field)
const char* const WL_FIELDS[] = {"A", "B", "C", "D", "part", "tmp", "tmp2", "res", "tree", "w", "trtop"};   // the write lists': fake(80 + i) (shim_wl_field)

fheram_ctx* make_path_ctx(unsigned* host_words, int lg, int ws, int s_evk, const Setting& st) {
    fheram_ctx* c = make_ctx(host_words);
    c->cus = 256; c->s_evk = s_evk; c->atk = (size_t)fheram_ctx::DNUM_CT * s_evk * 2 * N;
    c->ws = ws; c->rows = c->rows_glob = (size_t)1 << (lg - LOGN);
    c->base2d.clear();
    for (int bits = lg; bits != 0;) {   // get_base_2d with DECOMP_N = [3, 3, 3, 3] (fheram_ctx_create_cfg)
        std::vector<int> v;
        for (int i = 0; i < 4; i++) {
            if (3 <= bits) { v.push_back(3); bits -= 3; }
            else { if (bits != 0) { v.push_back(bits); bits = 0; } break; }
        }
        c->base2d.push_back(v);
    }
    c->n2 = (int)c->base2d.size();
    for (auto& v : c->base2d) { c->n_digits += (int)v.size(); c->max_digits = std::max(c->max_digits, (int)v.size()); }
    c->d_prep_inv = fake<double*>(14); c->d_ggsw_tmp = fake<int32_t*>(15); c->d_ggsw_tmp2 = fake<int32_t*>(16); c->d_ggsw_inv = fake<int32_t*>(17);
    c->d_atk_inv = fake<double*>(18); c->d_tsk = fake<double*>(19);
    c->ev_fork = fake<hipEvent_t>(20); c->ev_join = fake<hipEvent_t>(21); c->ev_inv[0] = fake<hipEvent_t>(22); c->ev_inv[1] = fake<hipEvent_t>(23);
    c->ev_wdone = fake<hipEvent_t>(24); c->ev_opstart = fake<hipEvent_t>(25);
    shim_batch_prep(c, fake<double*>(26));
    for (int i = 0; i < 12; i++) c->*FIELDS[i].p = arena(i);
    for (int i = 0; i < 6; i++) shim_batch_field(c, i) = arena(16 + i);
    c->keys_loaded = true;
    c->cur = c->stream;
    st.apply(c);
    return c;
}
fheram_addr* make_addr(fheram_ctx* c, int k) { return new fheram_addr{c, fake<int32_t*>(56 + k), c->n_digits, 0}; }

uint64_t path_ops = 0;
void op(const std::string& what) { path_ops++; ll::line(what); }
// what an operation left in the context: its own RAM state, the flags of the write in flight, every buffer field and the word count
void dump_ctx(const fheram_ctx* c) {
    const ShimState s = shim_state(c);
    char buf[160];
    std::snprintf(buf, sizeof buf, "  -> ctx state=%d memo_top=%d memo_alone=%d res_in_trtop=%d | side_begun=%d trhi=%c rotate_pending=%d words_staged=%d | ws=%d", s.state,
                  s.memo_top, s.memo_alone, s.res_in_trtop, c->side_begun, c->side_begun ? shim_trhi(c) : '-', c->tree_rotate_pending, c->words_staged, c->ws);
    std::string l = buf;
    for (const Field& f : FIELDS) l += std::string(" ") + f.name + "=" + ll::arena_of((uint64_t)(uintptr_t)(c->*f.p));
    ll::line(l);
}
bool dump_wl = false;   // from the first write list on: what the bank remembers of the lists' arena
void dump_bank(const fheram_bank* b) {
    if (dump_wl) ll::line("  -> " + shim_wl_kept(b));
    for (int m = 0; m < b->M; m++) {
        const ShimState s = shim_state(b, m);
        char buf[128];
        std::snprintf(buf, sizeof buf, "  -> member %d state=%d memo_top=%d memo_alone=%d res_in_trtop=%d", m, s.state, s.memo_top, s.memo_alone, s.res_in_trtop);
        ll::line(buf);
    }
    dump_ctx(b->c);
}
// where the words of a write are staged, between the side stage and the top: the destination, the count, the flags of the write in flight
auto staging(fheram_ctx* c, int rc) {
    return [c, rc](const int32_t* d_w, int n_ct) {
        char buf[128];
        std::snprintf(buf, sizeof buf, "  word stage -> %s, %d ciphertexts%s | side_begun=%d trhi=%c", ll::arena_of((uint64_t)(uintptr_t)d_w).c_str(), n_ct,
                      rc == FHERAM_OK ? "" : " (refused)", c->side_begun, c->n2 == 2 ? shim_trhi(c) : '-');
        ll::line(buf);
        return rc;
    };
}
void synced(fheram_ctx* c) { c->wide_unsynced = false; }   // the host has waited for the stream (a result download)

void run_path_ctx(fheram_ctx* c) {
    const fheram_addr* a[4];
    for (int k = 0; k < 4; k++) a[k] = make_addr(c, k);
    shim_loaded(c);
    op("ctx read a0"); shim_read(c, a[0], false); dump_ctx(c); synced(c);
    op("ctx read_prepare_write a0"); shim_read(c, a[0], true); dump_ctx(c); synced(c);
    op("ctx write a0"); shim_write(c, a[0], staging(c, FHERAM_OK)); dump_ctx(c);
    op("ctx read_prepare_write a1 (the host does not wait)"); shim_read(c, a[1], true); dump_ctx(c);
    op("ctx write a1 after a key load"); shim_new_keys(c); c->inv_id[0] = c->inv_id[1] = 0; c->inv_pending[0] = c->inv_pending[1] = false;
    shim_write(c, a[1], staging(c, FHERAM_OK)); dump_ctx(c);
    op("ctx read a0"); shim_read(c, a[0], false); dump_ctx(c); synced(c);
    for (int K = 2; K <= 4; K += 2) {
        op("ctx read_batch K=" + std::to_string(K));
        shim_batch_field(c, 2) = shim_needs_third(c, K) ? arena(18) : nullptr;   // (as the reserve allocates it)
        shim_batch(c, a, K);
        dump_ctx(c); synced(c);
    }
    // a batch the host does not wait for, then a gated read_prepare_write: whether that one records ev_opstart (ctx.hpp wide_unsynced)
    op("ctx read_batch K=2 (the host does not wait)");
    shim_batch_field(c, 2) = shim_needs_third(c, 2) ? arena(18) : nullptr;
    shim_batch(c, a, 2); dump_ctx(c);
    op("ctx read_prepare_write a0 behind it"); shim_read(c, a[0], true); dump_ctx(c); synced(c);
    op("ctx write a0"); shim_write(c, a[0], staging(c, FHERAM_OK)); dump_ctx(c);
    for (int k = 0; k < 4; k++) delete a[k];
}
void bank_step(fheram_bank* b, int first, int n, const fheram_addr* const* a, int stage_rc = FHERAM_OK) {
    const std::string r = " [" + std::to_string(first) + ", " + std::to_string(first + n) + ")";
    op("bank read_prepare_write" + r); shim_bank_read(b, first, n, a, true); dump_bank(b); synced(b->c);
    if (stage_rc != FHERAM_OK) { op("bank write" + r + ", words refused"); shim_bank_write(b, first, n, a, staging(b->c, stage_rc)); dump_bank(b); }
    op("bank write" + r); shim_bank_write(b, first, n, a, staging(b->c, FHERAM_OK)); dump_bank(b);
    op("bank read" + r); shim_bank_read(b, first, n, a, false); dump_bank(b); synced(b->c);
}
// read_prepare_write / write on any member set of the bank of three: every path a list can take (kept rows, gather, refusal, range <-> list,
// a read list between the halves); the host has waited (a result download) where `waited` says so, which is what lets a write skip its fork event
std::string list_name(const int* m, int n) {
    std::string s = "[";
    for (int k = 0; k < n; k++) s += (k ? "," : "") + std::to_string(m[k]);
    return s + "]";
}
void rpw_list(fheram_bank* b, const int* m, const fheram_addr* const* a, int n, bool waited = true) {
    op("bank read_prepare_write_list " + list_name(m, n)); shim_bank_rpw_list(b, m, a, n); dump_bank(b); synced(b->c);
    if (waited) main_waited(b->c);
}
void write_list(fheram_bank* b, const int* m, const fheram_addr* const* a, int n, int stage_rc = FHERAM_OK) {
    op("bank write_list " + list_name(m, n) + (stage_rc != FHERAM_OK ? ", words refused" : "")); shim_bank_write_list(b, m, a, n, staging(b->c, stage_rc)); dump_bank(b);
}
void run_path_write_lists(fheram_bank* b, const fheram_addr* const* a) {
    fheram_ctx* c = b->c;
    dump_wl = true;
    shim_wl_cap(b, 3);
    for (int i = 0; i < 11; i++) shim_wl_field(b, i) = fake<int32_t*>(80 + i);
    const int l20[] = {2, 0}, l02[] = {0, 2}, l10[] = {1, 0}, l210[] = {2, 1, 0}, l012[] = {0, 1, 2}, l11[] = {1, 1};
    const fheram_addr* a2[] = {a[2], a[0]}, *a1[] = {a[1], a[1]};
    // the same members in the same order: the rows are kept, nothing is gathered
    rpw_list(b, l20, a2, 2); write_list(b, l20, a2, 2);
    // permuted: a gather, and the kept rows do not count
    rpw_list(b, l20, a2, 2); write_list(b, l02, a, 2);
    // a range pending across a list; the list's words refused, then accepted
    op("bank read_prepare_write [1, 2)"); shim_bank_read(b, 1, 1, a + 1, true); dump_bank(b); synced(c);
    rpw_list(b, l02, a, 2); write_list(b, l02, a, 2, FHERAM_ERR_RANGE); write_list(b, l02, a, 2);
    op("bank write [1, 2)"); shim_bank_write(b, 1, 1, a + 1, staging(c, FHERAM_OK)); dump_bank(b);
    // prepared by range, written by list, and the other way round (a list of a contiguous ascending run IS the range)
    op("bank read_prepare_write [0, 2)"); shim_bank_read(b, 0, 2, a, true); dump_bank(b); synced(c); main_waited(c);
    write_list(b, l10, a, 2);
    rpw_list(b, l210, a, 3);
    op("bank write [0, 3)"); shim_bank_write(b, 0, 3, a, staging(c, FHERAM_OK)); dump_bank(b);
    rpw_list(b, l012, a, 3); write_list(b, l012, a, 3);
    // a read list between the two halves touches nothing of the lists'
    rpw_list(b, l20, a2, 2);
    op("bank read_list [1, 1]"); shim_list_field(b, 2) = third_arena_needed(c, 2 * b->mws) ? fake<int32_t*>(66) : nullptr; shim_bank_list(b, l11, a1, 2); dump_bank(b); synced(c); main_waited(c);
    write_list(b, l20, a2, 2);
}
void run_path_bank(fheram_ctx* c, int M, int mws) {
    fheram_bank* b = new fheram_bank();
    b->c = c; b->M = M; b->mws = mws;
    b->d_prep = fake<double*>(60); b->d_prep_inv = fake<double*>(61);
    if (M > 1) c->cfg.pre_inv = 0;   // (fheram_bank_create)
    shim_loaded(b);
    const fheram_addr* a[3];
    for (int k = 0; k < 3; k++) a[k] = make_addr(c, k);
    ll::line("bank M=" + std::to_string(M));
    bank_step(b, 0, M, a, M == 2 ? FHERAM_ERR_RANGE : FHERAM_OK);
    if (M == 3) {
        bank_step(b, 1, 1, a + 1);   // one member: the plain operation, memo kept
        bank_step(b, 1, 2, a + 1);
        op("bank read_prepare_write [0, 1)"); shim_bank_read(b, 0, 1, a, true); dump_bank(b); synced(c);
        op("bank read_prepare_write [1, 3)"); shim_bank_read(b, 1, 2, a + 1, true); dump_bank(b); synced(c);
        op("bank write [0, 3) over both"); shim_bank_write(b, 0, 3, a, staging(c, FHERAM_OK)); dump_bank(b);
        op("bank read [2, 3)"); shim_bank_read(b, 2, 1, a + 2, false); dump_bank(b); synced(c);
        // read lists: a permutation, and repeats over all three members
        shim_list_prep(b, fake<double*>(70));
        for (int i = 0; i < 6; i++) shim_list_field(b, i) = fake<int32_t*>(64 + i);
        const int perm[] = {1, 0}, rep[] = {0, 0, 1, 2};
        const fheram_addr* la[] = {a[0], a[1], a[2], a[0]};
        for (int n : {2, 4}) {
            if ((long)n * mws > 64) continue;
            op(n == 2 ? "bank read_list [1, 0]" : "bank read_list [0, 0, 1, 2]");
            shim_list_field(b, 2) = third_arena_needed(c, n * mws) ? fake<int32_t*>(66) : nullptr;   // (as the reserve allocates it)
            shim_bank_list(b, n == 2 ? perm : rep, la, n); dump_bank(b); synced(c);
        }
    }
    if (M == 3) run_path_write_lists(b, a);
    dump_wl = false;
    for (int k = 0; k < 3; k++) delete a[k];
    delete b;
}

// ---- the refusals: the bank's checks (not the entry points) with each bad argument of the range, read-list and write-list forms --------
// Bank of three, member 1 between read_prepare_write and write.  One line per case: the code, the message (fheram_bank_last_error's text) and
// how often the mid re-arm counted the call.
template <typename F>
void refuse(fheram_bank* b, const std::string& what, F&& check) {
    fheram_ctx* c = b->c;
    c->err.clear(); c->cfg.mid = 0; c->mid_saved = 2; c->mid_off_ops = 0;
    const bool verbose = ll::verbose;
    ll::verbose = false;   // (an accepted call enqueues: its launches are not part of the refusal log)
    const int rc = check();
    ll::verbose = verbose;
    ll::line(what + " -> " + std::to_string(rc) + " \"" + c->err + "\" rearm=" + std::to_string(c->mid_off_ops));
}
void run_refusals(unsigned* host_words) {
    std::puts("# refusals: bank of three, word_size 2, member 1 pending; <case> -> <code> \"<message>\" rearm=<mid re-arm count>");
    fheram_ctx* c = make_path_ctx(host_words, 13, 3 * 2, 4, PATH_SETTINGS[0]);
    fheram_ctx* other = make_path_ctx(host_words, 13, 3 * 2, 4, PATH_SETTINGS[0]);
    fheram_bank* b = new fheram_bank();
    b->c = c; b->M = 3; b->mws = 2;
    const fheram_addr* a[3];
    for (int k = 0; k < 3; k++) a[k] = make_addr(c, k);
    fheram_addr* foreign = make_addr(other, 0);
    fheram_addr* empty = make_addr(c, 3);
    empty->empty = true;
    const int m012[] = {0, 1, 2}, m02[] = {0, 2}, m1[] = {1}, neg[] = {0, -1}, big[] = {0, 3}, twice[] = {2, 0, 2}, m11[] = {1, 1}, nine[] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const fheram_addr *good[] = {a[0], a[1], a[2], a[0], a[1], a[2], a[0], a[1], a[2]}, *with_null[] = {a[0], nullptr, a[2]}, *with_foreign[] = {a[0], foreign, a[2]}, *with_empty[] = {a[0], empty, a[2]};
    auto ready = [&] { shim_loaded(b); c->keys_loaded = true; for (int m = 0; m < 3; m++) shim_set_state(b, m, m == 1); };
    ready();
    for (int want : {0, 1, -1}) {
        const std::string w = want == 0 ? "range read" : want == 1 ? "range write" : "range result";
        refuse(b, w + " null bank", [&] { return shim_check_range(nullptr, 0, 1, good, false, want); });
        if (want >= 0) refuse(b, w + " null addrs", [&] { return shim_check_range(b, 0, 1, nullptr, false, want); });
        if (want == 1) refuse(b, w + " null words", [&] { return shim_check_range(b, 1, 1, good, true, want); });
        refuse(b, w + " n=0", [&] { return shim_check_range(b, 0, 0, good, false, want); });
        refuse(b, w + " n=4", [&] { return shim_check_range(b, 0, 4, good, false, want); });
        refuse(b, w + " first=-1", [&] { return shim_check_range(b, -1, 1, good, false, want); });
        refuse(b, w + " first=3", [&] { return shim_check_range(b, 3, 1, good, false, want); });
        refuse(b, w + " [2, 4)", [&] { return shim_check_range(b, 2, 2, good, false, want); });
        if (want >= 0) {
            refuse(b, w + " null address", [&] { return shim_check_range(b, 0, 3, with_null, false, want); });
            refuse(b, w + " foreign address", [&] { return shim_check_range(b, 0, 3, with_foreign, false, want); });
            refuse(b, w + " empty address", [&] { return shim_check_range(b, 0, 3, with_empty, false, want); });
        }
        shim_set_initialized(b, 2, false);
        refuse(b, w + " member 2 uninitialised", [&] { return shim_check_range(b, 0, 3, good, false, want); });
        ready(); c->keys_loaded = false;
        refuse(b, w + " no keys", [&] { return shim_check_range(b, 0, 1, good, false, want); });
        ready();
        refuse(b, w + " [0, 3) over the pending member", [&] { return shim_check_range(b, 0, 3, good, false, want); });
        refuse(b, w + " [1, 2) the pending member", [&] { return shim_check_range(b, 1, 1, good, false, want); });
        refuse(b, w + " [2, 3) accepted or not", [&] { return shim_check_range(b, 2, 1, good, false, want); });
    }
    refuse(b, "read list null bank", [&] { return shim_check_rlist(nullptr, m02, good, 2); });
    refuse(b, "read list null members", [&] { return shim_check_rlist(b, nullptr, good, 2); });
    refuse(b, "read list null addrs", [&] { return shim_check_rlist(b, m02, nullptr, 2); });
    refuse(b, "read list n=0", [&] { return shim_check_rlist(b, m02, good, 0); });
    refuse(b, "read list n=9", [&] { return shim_check_rlist(b, nine, good, 9); });
    refuse(b, "read list member -1", [&] { return shim_check_rlist(b, neg, good, 2); });
    refuse(b, "read list member 3", [&] { return shim_check_rlist(b, big, good, 2); });
    refuse(b, "read list null address", [&] { return shim_check_rlist(b, m012, with_null, 3); });
    refuse(b, "read list foreign address", [&] { return shim_check_rlist(b, m012, with_foreign, 3); });
    refuse(b, "read list empty address", [&] { return shim_check_rlist(b, m012, with_empty, 3); });
    shim_set_initialized(b, 2, false);
    refuse(b, "read list member 2 uninitialised", [&] { return shim_check_rlist(b, twice, good, 3); });
    ready(); c->keys_loaded = false;
    refuse(b, "read list no keys", [&] { return shim_check_rlist(b, m02, good, 2); });
    ready();
    refuse(b, "read list [1,1] the pending member", [&] { return shim_check_rlist(b, m11, good, 2); });
    refuse(b, "read list [2,0,2] accepted", [&] { return shim_check_rlist(b, twice, good, 3); });
    b->mws = 16;   // (a bank of 3 x 16 = 48 ciphertexts)
    refuse(b, "read list n * word_size = 80", [&] { return shim_check_rlist(b, nine, good, 5); });
    b->mws = 2;
    for (int want : {0, 1}) {
        const std::string w = want == 0 ? "read_prepare_write list" : "write list";
        refuse(b, w + " null bank", [&] { return shim_check_wlist(nullptr, m02, good, 2, false, want); });
        refuse(b, w + " null members", [&] { return shim_check_wlist(b, nullptr, good, 2, false, want); });
        refuse(b, w + " null addrs", [&] { return shim_check_wlist(b, m02, nullptr, 2, false, want); });
        if (want == 1) refuse(b, w + " null words", [&] { return shim_check_wlist(b, m1, good, 1, true, want); });
        refuse(b, w + " n=0", [&] { return shim_check_wlist(b, m02, good, 0, false, want); });
        refuse(b, w + " n=4", [&] { return shim_check_wlist(b, nine, good, 4, false, want); });
        refuse(b, w + " member -1", [&] { return shim_check_wlist(b, neg, good, 2, false, want); });
        refuse(b, w + " member 3", [&] { return shim_check_wlist(b, big, good, 2, false, want); });
        refuse(b, w + " member 2 twice", [&] { return shim_check_wlist(b, twice, good, 3, false, want); });
        refuse(b, w + " null address", [&] { return shim_check_wlist(b, m012, with_null, 3, false, want); });
        refuse(b, w + " foreign address", [&] { return shim_check_wlist(b, m012, with_foreign, 3, false, want); });
        refuse(b, w + " empty address", [&] { return shim_check_wlist(b, m012, with_empty, 3, false, want); });
        shim_set_initialized(b, 2, false);
        refuse(b, w + " member 2 uninitialised", [&] { return shim_check_wlist(b, m02, good, 2, false, want); });
        ready(); c->keys_loaded = false;
        refuse(b, w + " no keys", [&] { return shim_check_wlist(b, m02, good, 2, false, want); });
        ready();
        refuse(b, w + " [0,2]", [&] { return shim_check_wlist(b, m02, good, 2, false, want); });
        refuse(b, w + " [1]", [&] { return shim_check_wlist(b, m1, good, 1, false, want); });
        refuse(b, w + " [0,1,2]", [&] { return shim_check_wlist(b, m012, good, 3, false, want); });
    }
    for (int k = 0; k < 3; k++) delete a[k];
    delete foreign; delete empty; delete b; delete c; delete other;
}

// ---- the reserve log: what a sequence of reserves allocates, frees and waits for, and what the set holds afterwards ----------------------
// 2^13, word_size 2 (two rows: n * ws <= 4 ciphertexts take the tail chain on the rows, so n = 2 needs the third arena and n = 3 does not)
void run_reserves(unsigned* host_words) {
    std::puts("# reserves: 2^13, word_size 2; one line per call: every allocation (bytes), free and stream wait in order, then the code, the message, the capacity and the buffers held");
    ll::reserve_mode = true;
    (void)ll::take_events();
    fheram_ctx* c = make_path_ctx(host_words, 13, 2, 4, PATH_SETTINGS[0]);
    auto reads = [&](ShimReadSet& L, int n, int fail_nth) {
        ll::fail_nth = fail_nth; c->err.clear();
        const int rc = shim_reads_reserve(c, L, n, c->ws);
        ll::fail_nth = 0;
        ll::line("read set: reserve n=" + std::to_string(n) + (fail_nth ? ", allocation " + std::to_string(fail_nth) + " fails" : "") + ": " + ll::take_events() + " -> " +
                 std::to_string(rc) + " \"" + c->err + "\" " + shim_reads_holds(L));
    };
    {
        ShimReadSet L;
        for (int n : {1, 3, 2, 3, 1}) reads(L, n, 0);
        shim_reads_free(L); ll::line("read set: free: " + ll::take_events() + " -> " + shim_reads_holds(L));
        for (int nth : {1, 4, 7}) {
            reads(L, 3, nth);                    // a fresh set
            reads(L, 1, 0); reads(L, 3, nth);    // growth
            reads(L, 3, 0); reads(L, 2, nth);   // the third arena alone, the capacity kept
            shim_reads_free(L); ll::line("read set: free: " + ll::take_events());
        }
    }
    fheram_ctx* c3 = make_path_ctx(host_words, 13, 3 * 2, 4, PATH_SETTINGS[0]);
    fheram_bank* b = new fheram_bank();
    b->c = c3; b->M = 3; b->mws = 2;
    auto wl = [&](int n, int nth) {
        fheram_bank_selftest_fail_list_alloc(b, nth); c3->err.clear();
        const int rc = shim_wl_reserve(b, n);
        ll::line("write-list set: reserve n=" + std::to_string(n) + (nth ? ", fail_list_alloc " + std::to_string(nth) : "") + ": " + ll::take_events() + " -> " + std::to_string(rc) +
                 " \"" + c3->err + "\" " + shim_wl_holds(b));
    };
    for (int n : {2, 3, 2}) wl(n, 0);
    shim_wl_free(b); ll::line("write-list set: free: " + ll::take_events() + " -> " + shim_wl_holds(b));
    for (int nth : {1, 5, 11, 12}) {
        wl(3, nth);              // a fresh set (12: one more than the set has, so it stays armed)
        wl(2, 0); wl(3, nth);    // growth
        shim_wl_free(b); ll::line("write-list set: free: " + ll::take_events());
        fheram_bank_selftest_fail_list_alloc(b, 0);
    }
    ll::reserve_mode = false;
    delete b; delete c3; delete c;
}

int path_main(long only, unsigned* host_words) {
    ll::path_mode = true;
    if (only < 0) {
        std::string legend = "# arenas:";
        for (int i = 0; i < 12; i++) legend += std::string(" a") + std::to_string(32 + i) + "=" + FIELDS[i].name;
        for (int i = 0; i < 6; i++) legend += std::string(" a") + std::to_string(48 + i) + "=batch." + READS_FIELDS[i];
        for (int i = 0; i < 6; i++) legend += std::string(" a") + std::to_string(64 + i) + "=list." + READS_FIELDS[i];
        for (int i = 0; i < 11; i++) legend += std::string(" a") + std::to_string(80 + i) + "=wl." + WL_FIELDS[i];
        std::puts(legend.c_str());
        std::puts("# a13=prep a14=prep_inv a15=ggsw_tmp a16=ggsw_tmp2 a17=ggsw_inv a26=batch.prep a56..=address digits a60=bank prep a61=bank prep_inv a70=list.prep; events: a20=fork a21=join a22,a23=inv a24=wdone a25=opstart");
    }
    long id = 0;
    for (int lg : PATH_LOG_MAX_ADDR) for (int ws : {1, 4}) for (int s_evk = 4; s_evk <= 5; s_evk++) for (const Setting& st : PATH_SETTINGS) {
        if (only >= 0 && id != only) { id++; continue; }
        ll::verbose = only >= 0;
        ll::digest = 0xcbf29ce484222325ull; ll::lines = 0; path_ops = 0;
        std::printf("config %ld: max_addr=2^%d word_size=%d s_evk=%d %s\n", id, lg, ws, s_evk, st.name);
        fheram_ctx* c = make_path_ctx(host_words, lg, ws, s_evk, st);
        run_path_ctx(c);
        delete c;
        for (int M = 1; M <= 3; M++) {
            c = make_path_ctx(host_words, lg, M * ws, s_evk, st);
            run_path_bank(c, M, ws);
            delete c;
        }
        std::printf("config %ld: %" PRIu64 " operations, %" PRIu64 " lines, digest %016" PRIx64 "\n", id, path_ops, ll::lines, ll::digest);
        id++;
    }
    if (only < 0) { ll::verbose = true; run_refusals(host_words); run_reserves(host_words); }
    return 0;
}

// ---- onerow mode: the operations that keep last outputs, stage host words and read one-row RAMs, on a bank of two ------------------------
// select, select_lanes, the register file, the tables, the mixes, peek and poke through their ENTRY POINTS (the launchers of the other
// translation units are recorders), each followed by the return code, what it allocated, the members, every kind's last-outputs record, the
// pointer select_source gives for index 0 of every kind, the host stages' busy flags and a digest of what is staged.
struct OneRow {
    fheram_bank* b;
    fheram_ctx* c;
    const fheram_addr* a[3];
    std::vector<int64_t> words, bad_words, out;
    fheram_fheuint* fu;
};
OneRow make_onerow(unsigned* host_words, int lg, int ws, const Setting& st) {
    OneRow w;
    fheram_ctx* c = make_path_ctx(host_words, lg, 2 * ws, 4, st);
    c->p.n_decomp = 4; c->p.max_addr = (uint64_t)1 << lg; c->p.k_glwe_pt = 3; c->p.word_size = (uint32_t)(2 * ws);
    for (int i = 0; i < 4; i++) c->p.decomp_n[i] = 3;
    c->cfg.pre_inv = 0;   // (fheram_bank_create)
    c->h_w = new int32_t[64 * fheram_ctx::GLWE]();   // stage_words narrows into it (leaked with the configuration)
    c->ev_w = fake<hipEvent_t>(29);
    w.c = c;
    w.b = new fheram_bank();
    w.b->c = c; w.b->M = 2; w.b->mws = ws;
    w.b->d_prep = fake<double*>(60); w.b->d_prep_inv = fake<double*>(61);
    shim_loaded(w.b);
    for (int k = 0; k < 3; k++) w.a[k] = make_addr(c, k);
    const size_t per = (size_t)ws * fheram_ctx::GLWE;
    w.words.resize(40 * per);
    for (size_t i = 0; i < w.words.size(); i++) w.words[i] = (int64_t)(i % 2001) - 1000;
    w.bad_words = w.words;
    w.bad_words[per + 5] = 65537;   // slot 1, ciphertext 0
    w.out.assign(120 * fheram_ctx::GLWE, 0);
    w.fu = new fheram_fheuint{c, 0, 32, fake<int32_t*>(27), fake<double*>(28)};
    return w;
}
void free_onerow(OneRow& w) {
    shim_release(w.b);
    for (int k = 0; k < 3; k++) delete w.a[k];
    delete w.fu; delete w.b; delete w.c;
    (void)ll::take_events();
}
const char* const KIND_NAMES[] = {"list", "select", "regs", "table", "peek"};
void dump_last(const fheram_bank* b) {
    std::string l = "  -> last";
    for (int k = 0; k < 5; k++) {
        const ShimLast r = shim_last(b, k);
        l += std::string(" ") + KIND_NAMES[k] + "{n=" + std::to_string(r.n);
        if (r.n) l += " res=" + ll::ptr_name(r.res) + " h=" + ll::ptr_name(r.h) + " slot=" + std::to_string(r.mix_slot);
        l += "}";
    }
    l += " regs_old=" + ll::ptr_name(shim_regs_old(b));
    ll::line(l);
    const int kinds[] = {FHERAM_SRC_ZERO, FHERAM_SRC_HOST, FHERAM_SRC_MEMBER_RESULT, FHERAM_SRC_LIST_RESULT, FHERAM_SRC_SELECT_RESULT, FHERAM_SRC_REGS_RESULT, FHERAM_SRC_REGS_OLD, FHERAM_SRC_TABLE_RESULT, FHERAM_SRC_PEEK_RESULT};
    const int has[] = {1, 0, 1, shim_last(b, 0).n, shim_last(b, 1).n, shim_last(b, 2).n, shim_regs_old(b) != nullptr, shim_last(b, 3).n, shim_last(b, 4).n};
    l = "  -> source[0]";
    for (int i = 0; i < 9; i++) l += " " + std::to_string(kinds[i]) + ":" + (has[i] ? ll::ptr_name(shim_source(b, kinds[i], 0)) : std::string("-"));
    ll::line(l);
    l = "  -> " + shim_busy(b) + " staged";
    ShimPinned pin[6];
    const int n = shim_pinned(b, pin);
    for (int i = 0; i < n; i++) {
        char buf[64];
        std::snprintf(buf, sizeof buf, " %s=%016" PRIx64, pin[i].name, pin[i].p ? ll::fnv(0xcbf29ce484222325ull, pin[i].p, pin[i].bytes) : (uint64_t)0);
        l += buf;
        if (pin[i].p && !std::strcmp(pin[i].name, "lanes")) ll::arenas_in(l, pin[i].p, 16 * SELECT_CAND_MAX * sizeof(void*));   // (the first 16 output ciphertexts' pointers)
    }
    ll::line(l);
}
template <typename F>
int step(OneRow& w, const std::string& what, F&& f) {
    op(what);
    w.c->err.clear();
    const int rc = f();
    ll::line("  -> rc=" + std::to_string(rc) + " \"" + w.c->err + "\" allocations: " + ll::take_events());
    dump_bank(w.b);
    dump_last(w.b);
    return rc;
}
std::string regs_state(const fheram_regs* r) { return " (register file: initialized=" + std::to_string(r->initialized) + " state=" + std::to_string(r->state) + " memo=" + std::to_string(r->memo) + ")"; }
using Src = fheram_select_src;
// selectors of `bits` bits, derived from bits [first_bit, ..) of the integer by the recorded k_cmux_chain
fheram_selector* new_selector(OneRow& w, int bits, int first_bit, bool wide = false) {
    fheram_selector* s = nullptr;
    if (wide) fheram_bank_table_selector_alloc(w.b, bits, &s); else fheram_bank_selector_alloc(w.b, bits, &s);
    const fheram_fheuint* fus[] = {w.fu};
    fheram_selector* sels[] = {s};
    if (s) fheram_bank_selector_derive(w.b, fus, &first_bit, 1, sels);
    return s;
}
void run_onerow(unsigned* host_words, int lg, int ws, const Setting& st) {
    OneRow w = make_onerow(host_words, lg, ws, st);
    fheram_bank* b = w.b;
    const int64_t* hw = w.words.data();
    int64_t* out = w.out.data();
    const int nmax = std::min(4, 64 / ws);   // entries a call of this word size may have
    op("selectors: bits 3 x2 (one digit), bits 5 x2 (two digits), a wide one of 7 bits (three digits)");
    fheram_selector *s3a = new_selector(w, 3, 0), *s3b = new_selector(w, 3, 3), *s5a = new_selector(w, 5, 6), *s5b = new_selector(w, 5, 11), *w7 = new_selector(w, 7, 16, true);
    ll::line("  -> allocations: " + ll::take_events());
    const int m10[] = {1, 0}, m1[] = {1}, m0[] = {0};
    const fheram_addr* a10[] = {w.a[1], w.a[0]};
    step(w, "bank read [0, 2)", [&] { return fheram_bank_read(b, 0, 2, w.a, nullptr); });
    step(w, "bank read_list [1, 0]", [&] { return fheram_bank_read_list(b, m10, a10, 2, out); });
    // ---- the register file ----
    fheram_regs *r3 = nullptr, *r5 = nullptr;
    step(w, "regs_create bits=3, bits=5", [&] { const int rc = fheram_bank_regs_create(b, 3, &r3); return rc ? rc : fheram_bank_regs_create(b, 5, &r5); });
    const Src pack8[] = {{FHERAM_SRC_HOST, 2}, {FHERAM_SRC_MEMBER_RESULT, 1}, {FHERAM_SRC_LIST_RESULT, 1}, {FHERAM_SRC_ZERO, 0}, {FHERAM_SRC_HOST, 0}, {FHERAM_SRC_HOST, 2}, {FHERAM_SRC_LIST_RESULT, 0}, {FHERAM_SRC_MEMBER_RESULT, 0}};
    step(w, "regs_pack r3 <- [host2, member1, list1, zero, host0, host2, list0, member0]", [&] { return fheram_bank_regs_pack(b, r3, 8, pack8, hw); });
    step(w, "regs_pack r5 <- [host2, member1, list1] (the host stage still busy)", [&] { return fheram_bank_regs_pack(b, r5, 3, pack8, hw); });
    const fheram_selector* s3[] = {s3a, s3b, s3a, s3b}, *s5[] = {s5a, s5b, s5b, s5a};
    step(w, "regs_read r3 x2 (one digit: no products in the tail)", [&] { return fheram_bank_regs_read(b, r3, s3, 2, out); });
    step(w, "regs_read r5 x" + std::to_string(nmax) + " (two digits), no download", [&] { return fheram_bank_regs_read(b, r5, s5, nmax, nullptr); });
    step(w, "regs_result [1, 2)", [&] { return fheram_bank_regs_result(b, 1, 1, out); });
    step(w, "regs_read_prepare_write r3" + regs_state(r3), [&] { return fheram_bank_regs_read_prepare_write(b, r3, s3a, out); });
    step(w, "regs_old_result", [&] { return fheram_bank_regs_old_result(b, out); });
    step(w, "regs_write r3 <- host1" + regs_state(r3), [&] { return fheram_bank_regs_write(b, r3, s3a, Src{FHERAM_SRC_HOST, 1}, hw); });
    step(w, "regs_read_prepare_write r5, no download" + regs_state(r5), [&] { return fheram_bank_regs_read_prepare_write(b, r5, s5a, nullptr); });
    step(w, "regs_write r5 <- regs_old after new keys (memo void)" + regs_state(r5), [&] { regs_keys_changed(b); return fheram_bank_regs_write(b, r5, s5a, Src{FHERAM_SRC_REGS_OLD, 0}, nullptr); });
    // ---- the tables ----
    fheram_table *t5a = nullptr, *t5b = nullptr, *t7 = nullptr;
    step(w, "table_create bits=5 x2, bits=7", [&] { int rc = fheram_bank_table_create(b, 5, &t5a); if (!rc) rc = fheram_bank_table_create(b, 5, &t5b); return rc ? rc : fheram_bank_table_create(b, 7, &t7); });
    std::vector<uint8_t> bytes((size_t)128 * ws);
    for (size_t i = 0; i < bytes.size(); i++) bytes[i] = (uint8_t)(i * 7 + 3);
    step(w, "table_load_plain t5a", [&] { return fheram_bank_table_load_plain(b, t5a, bytes.data(), (size_t)32 * ws); });
    step(w, "table_load_plain t5b (the stage still busy)", [&] { return fheram_bank_table_load_plain(b, t5b, bytes.data() + 5, (size_t)32 * ws); });
    step(w, "table_load_plain t7", [&] { return fheram_bank_table_load_plain(b, t7, bytes.data(), (size_t)128 * ws); });
    const fheram_table* t55[] = {t5a, t5b, t5b, t5a}, *t7s[] = {t7};
    const fheram_selector* w7s[] = {w7};
    step(w, "table_read [t5a, t5b]", [&] { return fheram_bank_table_read(b, t55, s5, 2, out); });
    step(w, "table_read [t7] (three digits), no download", [&] { return fheram_bank_table_read(b, t7s, w7s, 1, nullptr); });
    step(w, "table_result [0, 1)", [&] { return fheram_bank_table_result(b, 0, 1, out); });
    // ---- the public side ----
    const uint64_t pa[] = {5, (uint64_t)1 << (lg - 1), 5, 4097 % ((uint64_t)1 << lg)};
    const int pm[] = {0, 1, 1, 0};
    step(w, "peek [(0, 5), (1, 2^(lg-1))]", [&] { return fheram_bank_peek(b, pm, pa, 2, out); });
    step(w, "peek_result [1, 2)", [&] { return fheram_bank_peek_result(b, 1, 1, out); });
    // ---- the selects: every source kind ----
    const Src cand8[] = {{FHERAM_SRC_HOST, 1}, {FHERAM_SRC_MEMBER_RESULT, 0}, {FHERAM_SRC_LIST_RESULT, 1}, {FHERAM_SRC_REGS_RESULT, 1}, {FHERAM_SRC_REGS_OLD, 0}, {FHERAM_SRC_TABLE_RESULT, 0}, {FHERAM_SRC_PEEK_RESULT, 1}, {FHERAM_SRC_ZERO, 0}};
    const int n8[] = {8, 3, 2, 1};
    const fheram_selector* sel1[] = {s3a};
    step(w, "select x1 of [host1, member0, list1, regs1, regs_old, table0, peek1, zero]", [&] { return fheram_bank_select(b, sel1, n8, 1, cand8, hw, out); });
    const Src cand_again[] = {{FHERAM_SRC_SELECT_RESULT, 0}, {FHERAM_SRC_HOST, 3}, {FHERAM_SRC_HOST, 0}, {FHERAM_SRC_SELECT_RESULT, 0}, {FHERAM_SRC_HOST, 3}, {FHERAM_SRC_PEEK_RESULT, 0}, {FHERAM_SRC_SELECT_RESULT, 0}, {FHERAM_SRC_TABLE_RESULT, 0},
                              {FHERAM_SRC_REGS_RESULT, 0}, {FHERAM_SRC_SELECT_RESULT, 0}, {FHERAM_SRC_LIST_RESULT, 0}, {FHERAM_SRC_SELECT_RESULT, 0}, {FHERAM_SRC_REGS_OLD, 0}, {FHERAM_SRC_SELECT_RESULT, 0}};
    const int n_again[] = {3, 3, 4, 4};
    step(w, "select x2 (two digits) of [select0, host3, host0 | select0, host3, peek0]: the buffers grow, the last outputs move", [&] { return fheram_bank_select(b, s5, n_again, 2, cand_again, hw, nullptr); });
    step(w, "select_result [0, 2)", [&] { return fheram_bank_select_result(b, 0, 2, out); });
    if (nmax >= 4) step(w, "select x4 of 3, 3, 4, 4 candidates: the buffers grow again", [&] { return fheram_bank_select(b, s5, n_again, 4, cand_again, hw, out); });
    std::vector<fheram_select_lane> lanes;
    for (int j = 0; j < 8; j++)
        for (int l = 0; l < ws; l++) lanes.push_back(fheram_select_lane{cand8[j].kind, cand8[j].index, cand8[j].kind == FHERAM_SRC_ZERO ? 0 : (l + j) % ws, 0});
    lanes[1] = fheram_select_lane{FHERAM_SRC_SELECT_RESULT, 1, 0, 0};
    step(w, "select_lanes x1 of the eight kinds, lane (l + j) mod ws; lane 1 of candidate 0 from select1", [&] { return fheram_bank_select_lanes(b, sel1, n8, 1, lanes.data(), hw, out); });
    step(w, "select_lanes again (table and stage still busy), no download", [&] { return fheram_bank_select_lanes(b, sel1, n8 + 1, 1, lanes.data(), hw, nullptr); });
    const int picks[] = {0, 0};
    step(w, "read_prepare_write_list [1, 0]", [&] { return fheram_bank_read_prepare_write_list(b, m10, a10, 2, nullptr); });
    step(w, "write_list_selected [1, 0] <- select0, select0", [&] { return fheram_bank_write_list_selected(b, m10, a10, 2, picks); });
    // ---- the mixes: both top forms (the tail up to 8 ciphertexts with 0 or 2+ digits everywhere), empty groups after single calls ----
    fheram_mix_reads mr{};
    mr.members = m10; mr.addrs = a10; mr.tables = t55; mr.table_sels = s5; mr.regs = r5; mr.reg_sels = s5;
    auto mix = [&](int nl, int nt, int nr, bool dl) {
        mr.n_list = nl; mr.n_table = nt; mr.n_regs = nr;
        step(w, "read_mix list=" + std::to_string(nl) + " table=" + std::to_string(nt) + " regs=" + std::to_string(nr) + (dl ? "" : ", no download"),
             [&] { return fheram_bank_read_mix(b, &mr, dl ? out : nullptr, dl ? out + 26 * fheram_ctx::GLWE : nullptr, dl ? out + 52 * fheram_ctx::GLWE : nullptr); });
    };
    mix(0, 1, 1, true);       // the list keeps its own home
    mix(1, 0, 0, true);       // table and regs in mix slot 0: this one takes slot 1
    mix(0, 0, 1, false);      // list in 1, table in 0: slot 2
    if (nmax >= 4) mix(2, 1, 1, true);
    step(w, "table_read [t5a] (the kind goes home)", [&] { return fheram_bank_table_read(b, t55, s5, 1, nullptr); });
    mix(0, 1, 0, true);
    mr.regs = r3; mr.reg_sels = s3;
    mix(1, 0, 1, true);       // a one-digit selector: never the tail form
    mr.regs = r5; mr.reg_sels = s5;
    fheram_mix_prepares mp{};
    auto rpw_mix = [&](const char* what, int nl, int nt, int nr, const int* pmem, const fheram_addr* const* paddr, int np, fheram_regs* pr, const fheram_selector* ps) {
        mr.n_list = nl; mr.n_table = nt; mr.n_regs = nr;
        mp.members = pmem; mp.addrs = paddr; mp.n_list = np; mp.regs = pr; mp.reg_sel = ps;
        step(w, std::string("read_prepare_write_mix ") + what, [&] {
            const size_t G = fheram_ctx::GLWE;
            return fheram_bank_read_prepare_write_mix(b, &mr, &mp, out, out + 26 * G, out + 52 * G, out + 78 * G, out + 104 * G);
        });
    };
    rpw_mix("table=1 | prepare [1] in place, r5", 0, 1, 0, m1, w.a + 1, 1, r5, s5a);
    step(w, "write_list [1]", [&] { return fheram_bank_write_list(b, m1, w.a + 1, 1, hw); });
    step(w, "regs_write r5 <- select0" + regs_state(r5), [&] { return fheram_bank_regs_write(b, r5, s5a, Src{FHERAM_SRC_SELECT_RESULT, 0}, nullptr); });
    rpw_mix("no reads | prepare [1, 0] dense (the fourth result buffer)", 0, 0, 0, m10, a10, 2, nullptr, nullptr);
    step(w, "write_list [1, 0]", [&] { return fheram_bank_write_list(b, m10, a10, 2, hw); });
    rpw_mix("list=1 (member 1) | prepare [1] (the packed row moves out of the way), r3", 1, 0, 0, m1, w.a + 1, 1, r3, s3b);
    step(w, "write_list [1]", [&] { return fheram_bank_write_list(b, m1, w.a + 1, 1, hw); });
    step(w, "regs_write r3 <- peek0" + regs_state(r3), [&] { return fheram_bank_regs_write(b, r3, s3b, Src{FHERAM_SRC_PEEK_RESULT, 0}, nullptr); });
    // ---- peek and poke ----
    const Src poke_srcs[] = {{FHERAM_SRC_HOST, 3}, {FHERAM_SRC_PEEK_RESULT, 0}, {FHERAM_SRC_HOST, 1}, {FHERAM_SRC_HOST, 3}};
    step(w, "poke [(0, 5) <- host3, (1, 2^(lg-1)) <- peek0]: the peek's outputs flip", [&] { return fheram_bank_poke(b, pm, pa, 2, poke_srcs, hw); });
    step(w, "poke x" + std::to_string(nmax) + " (the stage still busy)", [&] { return fheram_bank_poke(b, pm, pa, nmax, poke_srcs, hw); });
    step(w, "peek x1, no download", [&] { return fheram_bank_peek(b, pm + 1, pa + 1, 1, nullptr); });
    std::vector<uint8_t> image((size_t)N * ws, 9);
    step(w, "ram_load_plain member 0, row 0", [&] { return fheram_bank_ram_load_plain(b, 0, 0, 1, image.data(), image.size()); });
    step(w, "regs_load_plain r3", [&] { return fheram_bank_regs_load_plain(b, r3, bytes.data(), (size_t)8 * ws); });
    (void)m0;
    fheram_regs_destroy(r3);
    ll::line("  regs_destroy r3 -> regs_old=" + ll::ptr_name(shim_regs_old(b)));
    fheram_regs_destroy(r5);
    ll::line("  regs_destroy r5 (the owner of the last read_prepare_write) -> regs_old=" + ll::ptr_name(shim_regs_old(b)));
    for (fheram_table* t : {t5a, t5b, t7}) fheram_table_destroy(t);
    for (fheram_selector* s : {s3a, s3b, s5a, s5b, w7}) fheram_selector_destroy(s);
    free_onerow(w);
}

// the refusals of those operations' checks: one line per case as in path mode.  Bank of two, word size 2, 2^13; `fresh`: nothing has run on it
void run_onerow_refusals(unsigned* host_words) {
    std::puts("# refusals: bank of two, word_size 2, 2^13; <case> -> <code> \"<message>\" rearm=<mid re-arm count>");
    OneRow w = make_onerow(host_words, 13, 2, PATH_SETTINGS[0]), o = make_onerow(host_words, 13, 2, PATH_SETTINGS[0]);
    fheram_bank *b = w.b, *ob = o.b;
    fheram_ctx* c = w.c;
    const int64_t *hw = w.words.data(), *bad = w.bad_words.data();
    int64_t* out = w.out.data();
    ll::verbose = false;
    fheram_selector *s3 = new_selector(w, 3, 0), *s3b = new_selector(w, 3, 3), *s5 = new_selector(w, 5, 6), *w7 = new_selector(w, 7, 16, true), *foreign = new_selector(o, 3, 0), *empty = nullptr, *f3 = nullptr, *fresh_sel = nullptr;
    fheram_bank_selector_alloc(b, 3, &empty);
    const int widths[] = {1, 1, 1}, first_bits[] = {0, 1, 2};
    fheram_bank_selector_alloc_fields(b, widths, 3, &f3);
    const fheram_fheuint* fus3[] = {w.fu, w.fu, w.fu};
    fheram_bank_selector_derive_fields(b, f3, fus3, first_bits);
    fheram_regs *r3 = nullptr, *r3_new = nullptr, *o_regs = nullptr;
    fheram_table *t3 = nullptr, *t5 = nullptr, *t_new = nullptr, *o_tab = nullptr;
    fheram_bank_regs_create(b, 3, &r3); fheram_bank_regs_create(b, 3, &r3_new); fheram_bank_regs_create(ob, 3, &o_regs);
    fheram_bank_table_create(b, 3, &t3); fheram_bank_table_create(b, 5, &t5); fheram_bank_table_create(b, 3, &t_new); fheram_bank_table_create(ob, 3, &o_tab);
    ll::verbose = true;
    const int one[] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    const std::vector<std::pair<const char*, const fheram_selector*>> bad_sels = {{"null", nullptr}, {"foreign", foreign}, {"empty", empty}, {"of 5 bits", s5}, {"of three fields", f3}};
    const fheram_selector* sels[9] = {s3, s3b, s3, s3b, s3, s3b, s3, s3b, s3};
    auto sel_with = [&](const fheram_selector* s) { static const fheram_selector* v[2]; v[0] = s3; v[1] = s; return v; };
    auto refuse_src = [&](const std::string& what, fheram_bank* bk, Src s, const int64_t* host) {
        refuse(b, "select " + what, [&] { return fheram_bank_select(bk, sels, one, 1, &s, host, nullptr); });
    };
    // 1. nothing has run: the five _result downloads and every kind a source may name
    refuse(b, "read_list_result null bank", [&] { return fheram_bank_read_list_result(nullptr, 0, 1, out); });
    refuse(b, "read_list_result null output", [&] { return fheram_bank_read_list_result(b, 0, 1, nullptr); });
    refuse(b, "read_list_result none has run", [&] { return fheram_bank_read_list_result(b, 0, 1, out); });
    refuse(b, "select_result null output", [&] { return fheram_bank_select_result(b, 0, 1, nullptr); });
    refuse(b, "select_result none has run", [&] { return fheram_bank_select_result(b, 0, 1, out); });
    refuse(b, "regs_result null output", [&] { return fheram_bank_regs_result(b, 0, 1, nullptr); });
    refuse(b, "regs_result none has run", [&] { return fheram_bank_regs_result(b, 0, 1, out); });
    refuse(b, "regs_old_result none has run", [&] { return fheram_bank_regs_old_result(b, out); });
    refuse(b, "table_result null output", [&] { return fheram_bank_table_result(b, 0, 1, nullptr); });
    refuse(b, "table_result none has run", [&] { return fheram_bank_table_result(b, 0, 1, out); });
    refuse(b, "peek_result null output", [&] { return fheram_bank_peek_result(b, 0, 1, nullptr); });
    refuse(b, "peek_result none has run", [&] { return fheram_bank_peek_result(b, 0, 1, out); });
    for (int kind : std::initializer_list<int>{FHERAM_SRC_LIST_RESULT, FHERAM_SRC_SELECT_RESULT, FHERAM_SRC_REGS_RESULT, FHERAM_SRC_REGS_OLD, FHERAM_SRC_TABLE_RESULT, FHERAM_SRC_PEEK_RESULT})
        refuse_src("source kind " + std::to_string(kind) + ", none has run", b, Src{kind, 0}, nullptr);
    refuse_src("member 0 has no result", b, Src{FHERAM_SRC_MEMBER_RESULT, 0}, nullptr);
    // 2. everything has run once (quietly): list of 2, select of 2, register read of 3, table read of 2, peek of 2, a register read_prepare_write
    ll::verbose = false;
    {
        const int m10[] = {1, 1};   // member 0 stays without a result
        const fheram_addr* a10[] = {w.a[1], w.a[0]};
        const Src z[] = {{FHERAM_SRC_ZERO, 0}, {FHERAM_SRC_ZERO, 0}};
        const fheram_table* tt[] = {t3, t3};
        const uint64_t pa[] = {1, 2};
        std::vector<uint8_t> bytes(64, 1);
        fheram_bank_read(b, 1, 1, w.a, nullptr);
        fheram_bank_read_list(b, m10, a10, 2, nullptr);
        fheram_bank_select(b, sels, one, 2, z, nullptr, nullptr);
        fheram_bank_regs_pack(b, r3, 1, z, nullptr);
        fheram_bank_regs_read(b, r3, sels, 3, nullptr);
        fheram_bank_regs_read_prepare_write(b, r3, s3, nullptr);
        fheram_bank_table_load_plain(b, t3, bytes.data(), 16);
        fheram_bank_table_load_plain(b, t5, bytes.data(), 64);
        fheram_bank_table_read(b, tt, sels, 2, nullptr);
        fheram_bank_peek(b, m10, pa, 2, nullptr);
        (void)ll::take_events();
    }
    ll::verbose = true;
    for (int kind = 0; kind < 5; kind++) {
        auto result = [&](int first, int n) {
            switch (kind) {
            case 0: return fheram_bank_read_list_result(b, first, n, out);
            case 1: return fheram_bank_select_result(b, first, n, out);
            case 2: return fheram_bank_regs_result(b, first, n, out);
            case 3: return fheram_bank_table_result(b, first, n, out);
            default: return fheram_bank_peek_result(b, first, n, out);
            }
        };
        const std::string k = std::string(KIND_NAMES[kind]) + " result ";
        refuse(b, k + "first=-1", [&] { return result(-1, 1); });
        refuse(b, k + "n=0", [&] { return result(0, 0); });
        refuse(b, k + "[1, 4)", [&] { return result(1, 3); });
        refuse(b, k + "[3, 4)", [&] { return result(3, 1); });
    }
    // the select's own arguments and selectors
    refuse(b, "select null bank", [&] { return fheram_bank_select(nullptr, sels, one, 1, nullptr, nullptr, nullptr); });
    refuse(b, "select null sources", [&] { return fheram_bank_select(b, sels, one, 1, nullptr, nullptr, nullptr); });
    const Src zero9[9] = {};
    refuse(b, "select n=0", [&] { return fheram_bank_select(b, sels, one, 0, zero9, nullptr, nullptr); });
    refuse(b, "select n=9", [&] { return fheram_bank_select(b, sels, one, 9, zero9, nullptr, nullptr); });
    b->mws = 13;
    refuse(b, "select n * word_size = 65", [&] { return fheram_bank_select(b, sels, one, 5, zero9, nullptr, nullptr); });
    b->mws = 2;
    refuse(b, "select selector 1 null", [&] { return fheram_bank_select(b, sel_with(nullptr), one, 2, zero9, nullptr, nullptr); });
    refuse(b, "select selector 1 foreign", [&] { return fheram_bank_select(b, sel_with(foreign), one, 2, zero9, nullptr, nullptr); });
    refuse(b, "select selector 1 empty", [&] { return fheram_bank_select(b, sel_with(empty), one, 2, zero9, nullptr, nullptr); });
    refuse(b, "select selector 1 wide", [&] { return fheram_bank_select(b, sel_with(w7), one, 2, zero9, nullptr, nullptr); });
    refuse(b, "select selector 1 of 5 bits", [&] { return fheram_bank_select(b, sel_with(s5), one, 2, zero9, nullptr, nullptr); });
    refuse(b, "select selector 1 of three fields", [&] { return fheram_bank_select(b, sel_with(f3), one, 2, zero9, nullptr, nullptr); });
    const int none[] = {0}, nine[] = {9};
    refuse(b, "select 0 candidates", [&] { return fheram_bank_select(b, sels, none, 1, zero9, nullptr, nullptr); });
    refuse(b, "select 9 candidates of 8", [&] { return fheram_bank_select(b, sels, nine, 1, zero9, nullptr, nullptr); });
    // every kind and index of a source
    refuse_src("host, null host_words", b, Src{FHERAM_SRC_HOST, 0}, nullptr);
    refuse_src("host slot -1", b, Src{FHERAM_SRC_HOST, -1}, hw);
    refuse_src("host slot 256", b, Src{FHERAM_SRC_HOST, 256}, hw);
    refuse_src("member -1", b, Src{FHERAM_SRC_MEMBER_RESULT, -1}, hw);
    refuse_src("member 2", b, Src{FHERAM_SRC_MEMBER_RESULT, 2}, hw);
    refuse_src("member 0 has no result", b, Src{FHERAM_SRC_MEMBER_RESULT, 0}, hw);
    for (int kind : std::initializer_list<int>{FHERAM_SRC_LIST_RESULT, FHERAM_SRC_SELECT_RESULT, FHERAM_SRC_REGS_RESULT, FHERAM_SRC_TABLE_RESULT, FHERAM_SRC_PEEK_RESULT}) {
        refuse_src("kind " + std::to_string(kind) + " index -1", b, Src{kind, -1}, hw);
        refuse_src("kind " + std::to_string(kind) + " index 2", b, Src{kind, 2}, hw);
        refuse_src("kind " + std::to_string(kind) + " index 3", b, Src{kind, 3}, hw);
    }
    refuse_src("regs_old index 1", b, Src{FHERAM_SRC_REGS_OLD, 1}, hw);
    for (int kind : {7, 9, 11, -1}) refuse_src("unknown kind " + std::to_string(kind), b, Src{kind, 0}, hw);
    c->keys_loaded = false;
    refuse_src("no keys", b, Src{FHERAM_SRC_ZERO, 0}, hw);
    c->keys_loaded = true;
    refuse_src("host slot 1 out of range", b, Src{FHERAM_SRC_HOST, 1}, bad);
    refuse_src("host slot 0 accepted", b, Src{FHERAM_SRC_HOST, 0}, bad);
    // lanes
    {
        fheram_select_lane l2[2] = {{FHERAM_SRC_HOST, 0, 0, 0}, {FHERAM_SRC_HOST, 0, 1, 0}};
        auto lanes = [&](const std::string& what, fheram_select_lane l1, const int64_t* host) {
            l2[1] = l1;
            refuse(b, "select_lanes " + what, [&] { return fheram_bank_select_lanes(b, sels, one, 1, l2, host, nullptr); });
        };
        refuse(b, "select_lanes null lanes", [&] { return fheram_bank_select_lanes(b, sels, one, 1, nullptr, hw, nullptr); });
        refuse(b, "select_lanes n=9", [&] { return fheram_bank_select_lanes(b, sels, one, 9, l2, hw, nullptr); });
        lanes("lane 1 host, null host_words", {FHERAM_SRC_HOST, 0, 1, 0}, nullptr);
        lanes("lane 1 list index 2", {FHERAM_SRC_LIST_RESULT, 2, 0, 0}, hw);
        lanes("lane 1 unknown kind", {7, 0, 0, 0}, hw);
        lanes("lane 1 reserved = 1", {FHERAM_SRC_HOST, 0, 1, 1}, hw);
        lanes("lane 1 names lane 2", {FHERAM_SRC_HOST, 0, 2, 0}, hw);
        lanes("lane 1 names lane -1", {FHERAM_SRC_LIST_RESULT, 0, -1, 0}, hw);
        lanes("lane 1 member 0 has no result", {FHERAM_SRC_MEMBER_RESULT, 0, 0, 0}, hw);
        lanes("lane 1 host slot 1 lane 0 out of range", {FHERAM_SRC_HOST, 1, 0, 0}, bad);
        lanes("lane 1 host slot 1 lane 1 accepted", {FHERAM_SRC_HOST, 1, 1, 0}, bad);
        c->keys_loaded = false;
        lanes("no keys", {FHERAM_SRC_ZERO, 0, 0, 0}, hw);
        c->keys_loaded = true;
    }
    refuse(b, "write_list_selected pick 2 of 1", [&] { const int m[] = {0}, p[] = {2}; return fheram_bank_write_list_selected(b, m, w.a, 1, p); });
    // the register file: handle, selectors, sources (a register file takes host slots [0, 32), and a pack needs no keys), state
    const Src h0{FHERAM_SRC_HOST, 0};
    refuse(b, "regs_pack null handle", [&] { return fheram_bank_regs_pack(b, nullptr, 1, &h0, hw); });
    refuse(b, "regs_pack foreign handle", [&] { return fheram_bank_regs_pack(b, o_regs, 1, &h0, hw); });
    refuse(b, "regs_pack null sources", [&] { return fheram_bank_regs_pack(b, r3_new, 1, nullptr, hw); });
    refuse(b, "regs_pack 0 candidates", [&] { return fheram_bank_regs_pack(b, r3_new, 0, &h0, hw); });
    refuse(b, "regs_pack 9 candidates of 8", [&] { return fheram_bank_regs_pack(b, r3_new, 9, &h0, hw); });
    auto pack_src = [&](const std::string& what, Src s, const int64_t* host) { refuse(b, "regs_pack " + what, [&] { return fheram_bank_regs_pack(b, r3_new, 1, &s, host); }); };
    pack_src("host, null host_words", h0, nullptr);
    pack_src("host slot 32", Src{FHERAM_SRC_HOST, 32}, hw);
    pack_src("host slot 256", Src{FHERAM_SRC_HOST, 256}, hw);
    pack_src("list index 2", Src{FHERAM_SRC_LIST_RESULT, 2}, hw);
    pack_src("member 0 has no result", Src{FHERAM_SRC_MEMBER_RESULT, 0}, hw);
    pack_src("host slot 1 out of range", Src{FHERAM_SRC_HOST, 1}, bad);
    refuse(b, "regs_pack on the pending register file", [&] { return fheram_bank_regs_pack(b, r3, 1, &h0, hw); });
    refuse(ob, "regs_pack a fresh bank's select result", [&] { const Src s{FHERAM_SRC_SELECT_RESULT, 0}; return fheram_bank_regs_pack(ob, o_regs, 1, &s, hw); });
    c->keys_loaded = false;
    pack_src("host slot 0 without keys, accepted", h0, hw);
    c->keys_loaded = true;
    refuse(b, "regs_read null handle", [&] { return fheram_bank_regs_read(b, nullptr, sels, 1, nullptr); });
    refuse(b, "regs_read null selectors", [&] { return fheram_bank_regs_read(b, r3_new, nullptr, 1, nullptr); });
    refuse(b, "regs_read n=0", [&] { return fheram_bank_regs_read(b, r3_new, sels, 0, nullptr); });
    refuse(b, "regs_read n=9", [&] { return fheram_bank_regs_read(b, r3_new, sels, 9, nullptr); });
    b->mws = 13;
    refuse(b, "regs_read n * word_size = 65", [&] { return fheram_bank_regs_read(b, r3_new, sels, 5, nullptr); });
    b->mws = 2;
    for (const auto& ns : bad_sels) {
        const char* name = ns.first; const fheram_selector* s = ns.second;
        refuse(b, std::string("regs_read selector 1 ") + name, [&] { return fheram_bank_regs_read(b, r3_new, sel_with(s), 2, nullptr); });
        if (s != f3) refuse(b, std::string("regs_read_prepare_write selector ") + name, [&] { return fheram_bank_regs_read_prepare_write(b, r3_new, s, nullptr); });
        if (s != f3) refuse(b, std::string("regs_write selector ") + name, [&] { return fheram_bank_regs_write(b, r3, s, h0, hw); });
    }
    refuse(b, "regs_read the pending register file", [&] { return fheram_bank_regs_read(b, r3, sels, 1, nullptr); });
    refuse(b, "regs_read_prepare_write the pending register file", [&] { return fheram_bank_regs_read_prepare_write(b, r3, s3, nullptr); });
    refuse(b, "regs_write a register file that is not pending", [&] { return fheram_bank_regs_write(b, r3_new, s3, h0, hw); });
    refuse(b, "regs_write host slot 32", [&] { return fheram_bank_regs_write(b, r3, s3, Src{FHERAM_SRC_HOST, 32}, hw); });
    refuse(b, "regs_write table index 2", [&] { return fheram_bank_regs_write(b, r3, s3, Src{FHERAM_SRC_TABLE_RESULT, 2}, hw); });
    refuse(b, "regs_write host slot 1 out of range", [&] { return fheram_bank_regs_write(b, r3, s3, Src{FHERAM_SRC_HOST, 1}, bad); });
    c->keys_loaded = false;
    refuse(b, "regs_write no keys", [&] { return fheram_bank_regs_write(b, r3, s3, h0, hw); });
    refuse(b, "regs_read no keys", [&] { return fheram_bank_regs_read(b, r3_new, sels, 1, nullptr); });
    c->keys_loaded = true;
    r3_new->initialized = false;
    refuse(b, "regs_read uninitialised", [&] { return fheram_bank_regs_read(b, r3_new, sels, 1, nullptr); });
    refuse(b, "regs_download uninitialised", [&] { return fheram_bank_regs_download(b, r3_new, out); });
    refuse(b, "regs_download null handle", [&] { return fheram_bank_regs_download(b, nullptr, out); });
    refuse(b, "regs_download null row", [&] { return fheram_bank_regs_download(b, r3_new, nullptr); });
    refuse(b, "regs_upload foreign handle", [&] { return fheram_bank_regs_upload(b, o_regs, hw); });
    refuse(b, "regs_upload null row", [&] { return fheram_bank_regs_upload(b, r3_new, nullptr); });
    // the tables
    const fheram_table* t33[] = {t3, t3};
    auto tab_with = [&](const fheram_table* t) { static const fheram_table* v[2]; v[0] = t3; v[1] = t; return v; };
    refuse(b, "table_read null tables", [&] { return fheram_bank_table_read(b, nullptr, sels, 1, nullptr); });
    refuse(b, "table_read null selectors", [&] { return fheram_bank_table_read(b, t33, nullptr, 1, nullptr); });
    refuse(b, "table_read n=0", [&] { return fheram_bank_table_read(b, t33, sels, 0, nullptr); });
    refuse(b, "table_read n=9", [&] { return fheram_bank_table_read(b, t33, sels, 9, nullptr); });
    refuse(b, "table_read table 1 null", [&] { return fheram_bank_table_read(b, tab_with(nullptr), sels, 2, nullptr); });
    refuse(b, "table_read table 1 foreign", [&] { return fheram_bank_table_read(b, tab_with(o_tab), sels, 2, nullptr); });
    refuse(b, "table_read table 1 uninitialised", [&] { return fheram_bank_table_read(b, tab_with(t_new), sels, 2, nullptr); });
    for (const auto& ns : bad_sels)
        refuse(b, std::string("table_read selector 1 ") + ns.first, [&] { return fheram_bank_table_read(b, t33, sel_with(ns.second), 2, nullptr); });
    refuse(b, "table_read [t3, t5] with selectors of 1 and 2 digits", [&] { return fheram_bank_table_read(b, tab_with(t5), sel_with(s5), 2, nullptr); });
    c->keys_loaded = false;
    refuse(b, "table_read no keys", [&] { return fheram_bank_table_read(b, t33, sels, 1, nullptr); });
    c->keys_loaded = true;
    refuse(b, "table_download uninitialised", [&] { return fheram_bank_table_download(b, t_new, out); });
    refuse(b, "table_download null handle", [&] { return fheram_bank_table_download(b, nullptr, out); });
    refuse(b, "table_download null row", [&] { return fheram_bank_table_download(b, t3, nullptr); });
    refuse(b, "table_upload foreign handle", [&] { return fheram_bank_table_upload(b, o_tab, hw); });
    refuse(b, "table_upload null row", [&] { return fheram_bank_table_upload(b, t3, nullptr); });
    // the mixes: each group with the rules of its single call
    {
        const int m10[] = {1, 0}, m12[] = {1, 2};
        const fheram_addr* a10[] = {w.a[1], w.a[0]};
        fheram_mix_reads mr{};
        auto mix = [&](const std::string& what) { refuse(b, "read_mix " + what, [&] { return fheram_bank_read_mix(b, &mr, nullptr, nullptr, nullptr); }); };
        auto reset = [&] { mr = fheram_mix_reads{}; mr.members = m10; mr.addrs = a10; mr.tables = t33; mr.table_sels = sels; mr.regs = r3_new; mr.reg_sels = sels; };
        r3_new->initialized = true;
        reset(); mix("all groups empty");
        reset(); mr.n_table = 5; mr.n_regs = 4; mix("9 entries");
        reset(); mr.n_list = 1; mr.members = nullptr; mix("null member list");
        reset(); mr.n_list = 2; mr.members = m12; mix("list member 2");
        reset(); mr.n_table = 1; mr.tables = nullptr; mix("null table list");
        reset(); mr.n_table = 2; mr.tables = tab_with(nullptr); mix("table 1 null");
        reset(); mr.n_table = 2; mr.tables = tab_with(t_new); mix("table 1 uninitialised");
        for (const auto& ns : bad_sels) {
        const char* name = ns.first; const fheram_selector* s = ns.second;
            reset(); mr.n_table = 2; mr.table_sels = sel_with(s); mix(std::string("table selector 1 ") + name);
            reset(); mr.n_regs = 2; mr.reg_sels = sel_with(s); mix(std::string("register selector 1 ") + name);
        }
        reset(); mr.n_regs = 1; mr.regs = nullptr; mix("null register file");
        reset(); mr.n_regs = 1; mr.regs = o_regs; mix("foreign register file");
        reset(); mr.n_regs = 1; mr.reg_sels = nullptr; mix("null register selectors");
        reset(); mr.n_regs = 1; mr.regs = r3; mix("the pending register file");
        r3_new->initialized = false;
        reset(); mr.n_regs = 1; mix("uninitialised register file");
        r3_new->initialized = true;
        c->keys_loaded = false;
        reset(); mr.n_table = 1; mix("no keys");
        c->keys_loaded = true;
        fheram_mix_prepares mp{};
        auto rpw = [&](const std::string& what) { refuse(b, "read_prepare_write_mix " + what, [&] { return fheram_bank_read_prepare_write_mix(b, &mr, &mp, nullptr, nullptr, nullptr, nullptr, nullptr); }); };
        reset(); rpw("no preparation");
        reset(); mp.regs = r3; mp.reg_sel = s3; rpw("the pending register file");
        mp.regs = r3_new; mp.reg_sel = empty; rpw("empty selector");
        mp.reg_sel = s5; rpw("selector of 5 bits");
        mp.regs = o_regs; mp.reg_sel = s3; rpw("foreign register file");
        mp.regs = r3_new; mr.n_table = 2; mr.table_sels = sel_with(empty); rpw("table selector 1 empty");
        r3_new->initialized = false;
    }
    // the poke's sources (host slots [0, 16))
    {
        const int m[] = {1, 1};
        const uint64_t pa[] = {3, 4};
        auto poke = [&](const std::string& what, Src s, const int64_t* host) {
            const Src two[] = {{FHERAM_SRC_ZERO, 0}, s};
            refuse(b, "poke " + what, [&] { return fheram_bank_poke(b, m, pa, 2, two, host); });
        };
        refuse(b, "poke null sources", [&] { return fheram_bank_poke(b, m, pa, 2, nullptr, hw); });
        poke("source 1 host, null host_words", h0, nullptr);
        poke("source 1 host slot 16", Src{FHERAM_SRC_HOST, 16}, hw);
        poke("source 1 host slot 256", Src{FHERAM_SRC_HOST, 256}, hw);
        poke("source 1 peek index 2", Src{FHERAM_SRC_PEEK_RESULT, 2}, hw);
        poke("source 1 unknown kind", Src{7, 0}, hw);
        poke("source 1 member 0 has no result", Src{FHERAM_SRC_MEMBER_RESULT, 0}, hw);
        poke("source 1 host slot 1 out of range", Src{FHERAM_SRC_HOST, 1}, bad);
        refuse(ob, "poke a fresh bank's table result", [&] { const Src s[] = {{FHERAM_SRC_TABLE_RESULT, 0}, {FHERAM_SRC_ZERO, 0}}; return fheram_bank_poke(ob, m, pa, 2, s, hw); });
        c->keys_loaded = false;
        poke("no keys", h0, hw);
        c->keys_loaded = true;
    }
    // the selectors' three _create entry points and the two allocation forms
    {
        const int64_t* digits[3] = {hw, nullptr, hw};
        refuse(b, "selector_create null output", [&] { return fheram_bank_selector_create(b, digits, 1, 3, nullptr); });
        refuse(b, "selector_create null ggsw", [&] { return fheram_bank_selector_create(b, nullptr, 1, 3, &fresh_sel); });
        refuse(b, "selector_create bits=0", [&] { return fheram_bank_selector_create(b, digits, 1, 0, &fresh_sel); });
        refuse(b, "selector_create bits=6", [&] { return fheram_bank_selector_create(b, digits, 2, 6, &fresh_sel); });
        refuse(b, "selector_create 2 digits for 3 bits", [&] { return fheram_bank_selector_create(b, digits, 2, 3, &fresh_sel); });
        refuse(b, "selector_create null digit 0", [&] { return fheram_bank_selector_create(b, digits + 1, 1, 3, &fresh_sel); });
        refuse(b, "table_selector_create null ggsw", [&] { return fheram_bank_table_selector_create(b, nullptr, 1, 7, &fresh_sel); });
        refuse(b, "table_selector_create bits=13", [&] { return fheram_bank_table_selector_create(b, digits, 1, 13, &fresh_sel); });
        refuse(b, "table_selector_create 2 digits for 7 bits", [&] { return fheram_bank_table_selector_create(b, digits, 2, 7, &fresh_sel); });
        refuse(b, "table_selector_create null digit 0", [&] { return fheram_bank_table_selector_create(b, digits + 1, 3, 7, &fresh_sel); });
        const int wide_w[] = {3, 0, 3, 3, 3, 3}, long_w[] = {3, 3};
        refuse(b, "selector_create_fields null widths", [&] { return fheram_bank_selector_create_fields(b, digits, 1, nullptr, 1, &fresh_sel); });
        refuse(b, "selector_create_fields 0 fields", [&] { return fheram_bank_selector_create_fields(b, digits, 0, widths, 0, &fresh_sel); });
        refuse(b, "selector_create_fields 6 fields", [&] { return fheram_bank_selector_create_fields(b, digits, 6, wide_w, 6, &fresh_sel); });
        refuse(b, "selector_create_fields width 0", [&] { return fheram_bank_selector_create_fields(b, digits, 2, wide_w, 2, &fresh_sel); });
        refuse(b, "selector_create_fields 6 bits", [&] { return fheram_bank_selector_create_fields(b, digits, 2, long_w, 2, &fresh_sel); });
        refuse(b, "selector_create_fields 2 digits for 3 fields", [&] { return fheram_bank_selector_create_fields(b, digits, 2, widths, 3, &fresh_sel); });
        refuse(b, "selector_create_fields null digit 1", [&] { return fheram_bank_selector_create_fields(b, digits, 3, widths, 3, &fresh_sel); });
        refuse(b, "table_selector_alloc_fields 13 bits", [&] { const int v[] = {5, 5, 3}; return fheram_bank_table_selector_alloc_fields(b, v, 3, &fresh_sel); });
        refuse(b, "selector_download empty", [&] { return fheram_bank_selector_download(b, empty, out); });
        (void)ll::take_events();
    }
    ll::verbose = false;
    for (fheram_regs* r : {r3, r3_new, o_regs}) fheram_regs_destroy(r);
    for (fheram_table* t : {t3, t5, t_new, o_tab}) fheram_table_destroy(t);
    for (fheram_selector* s : {s3, s3b, s5, w7, foreign, empty, f3}) fheram_selector_destroy(s);
    free_onerow(w); free_onerow(o);
    ll::verbose = true;
}

// the reserve log of the one-row kinds: the first create or call of each kind, a select that grows twice, and the three self-test failing
// allocations at every nth.  One line per call, as in path mode, then what every buffer set of the bank holds.
void run_onerow_reserves(unsigned* host_words) {
    std::puts("# reserves: bank of two, word_size 2, 2^13; one line per call: every allocation (bytes), event, copy, free and wait in order, then the code, the message and what the bank's buffer sets hold");
    ll::reserve_mode = true;
    const Src z8[8] = {};
    const int one[] = {1, 1, 1, 1}, two[] = {2, 2, 2, 2};
    auto call = [&](OneRow& w, const std::string& what, auto&& f) {
        ll::verbose = false;
        w.c->err.clear();
        const int rc = f();
        ll::verbose = true;
        ll::line(what + ": " + ll::take_events() + " -> " + std::to_string(rc) + " \"" + w.c->err + "\" " + shim_sets(w.b));
    };
    const int m10[] = {1, 0}, m1[] = {1};
    const uint64_t pa[] = {1, 2};
    std::vector<uint8_t> bytes(64, 1);
    {
        OneRow w = make_onerow(host_words, 13, 2, PATH_SETTINGS[0]);
        fheram_bank* b = w.b;
        const fheram_addr* a10[] = {w.a[1], w.a[0]};
        ll::verbose = false;
        fheram_selector *s3 = new_selector(w, 3, 0), *s5 = new_selector(w, 5, 6);
        (void)ll::take_events();
        const fheram_selector *s3s[] = {s3, s3, s3, s3}, *s5s[] = {s5, s5, s5, s5};
        const Src host3[] = {{FHERAM_SRC_HOST, 0}, {FHERAM_SRC_HOST, 3}, {FHERAM_SRC_SELECT_RESULT, 0}, {FHERAM_SRC_HOST, 5}};
        fheram_regs* r = nullptr;
        fheram_table* t = nullptr;
        call(w, "select x1, no host candidate", [&] { return fheram_bank_select(b, s3s, one, 1, z8, nullptr, nullptr); });
        call(w, "select x1 again", [&] { return fheram_bank_select(b, s3s, one, 1, z8, nullptr, nullptr); });
        call(w, "select x2 with host slots 0 and 3: grows, the last output moves", [&] { return fheram_bank_select(b, s3s, two, 2, host3, w.words.data(), nullptr); });
        call(w, "select x4 of two digits, host slot 5: grows again", [&] { return fheram_bank_select(b, s5s, one, 4, host3, w.words.data(), nullptr); });
        call(w, "select x1: nothing to grow", [&] { return fheram_bank_select(b, s3s, one, 1, z8, nullptr, nullptr); });
        const fheram_select_lane l2[] = {{FHERAM_SRC_ZERO, 0, 0, 0}, {FHERAM_SRC_ZERO, 0, 0, 0}};
        call(w, "select_lanes x1: the pointer table", [&] { return fheram_bank_select_lanes(b, s3s, one, 1, l2, nullptr, nullptr); });
        call(w, "select_lanes x1 again", [&] { return fheram_bank_select_lanes(b, s3s, one, 1, l2, nullptr, nullptr); });
        call(w, "regs_create: the shared set and the register file's own", [&] { return fheram_bank_regs_create(b, 3, &r); });
        fheram_regs* r2 = nullptr;
        call(w, "regs_create again: the register file's own", [&] { return fheram_bank_regs_create(b, 5, &r2); });
        call(w, "table_create: the shared set and the row", [&] { return fheram_bank_table_create(b, 3, &t); });
        fheram_table* t2 = nullptr;
        call(w, "table_create again: the row", [&] { return fheram_bank_table_create(b, 3, &t2); });
        call(w, "table_load_plain", [&] { return fheram_bank_table_load_plain(b, t, bytes.data(), 16); });
        call(w, "regs_pack", [&] { return fheram_bank_regs_pack(b, r, 1, z8, nullptr); });
        call(w, "peek: the public side", [&] { return fheram_bank_peek(b, m10, pa, 2, nullptr); });
        call(w, "poke", [&] { return fheram_bank_poke(b, m10, pa, 2, host3, w.words.data()); });
        fheram_mix_reads mr{};
        const fheram_table* ts[] = {t};
        mr.members = m10; mr.addrs = a10; mr.n_list = 2; mr.tables = ts; mr.table_sels = s3s; mr.n_table = 1; mr.regs = r; mr.reg_sels = s3s; mr.n_regs = 1;
        call(w, "read_mix list=2 table=1 regs=1: the mix's set and the read list's", [&] { return fheram_bank_read_mix(b, &mr, nullptr, nullptr, nullptr); });
        fheram_mix_prepares mp{};
        mp.members = m1; mp.addrs = w.a + 1; mp.n_list = 1; mp.regs = r; mp.reg_sel = s3;
        call(w, "read_prepare_write_mix: what the prepares add", [&] { return fheram_bank_read_prepare_write_mix(b, &mr, &mp, nullptr, nullptr, nullptr, nullptr, nullptr); });
        call(w, "read_mix again", [&] { mr.n_list = 0; return fheram_bank_read_mix(b, &mr, nullptr, nullptr, nullptr); });
        ll::verbose = false;
        fheram_regs_destroy(r); fheram_regs_destroy(r2); fheram_table_destroy(t); fheram_table_destroy(t2);
        ll::verbose = true;
        ll::line("destroy of both register files and both tables: " + ll::take_events());
        shim_release(b);
        ll::line("release of the bank's sets: " + ll::take_events() + " -> " + shim_sets(b));
        ll::verbose = false;
        fheram_selector_destroy(s3); fheram_selector_destroy(s5);
        free_onerow(w);
    }
    // the self-test's failing allocations: a fresh bank for every nth, the call that reserves, then the same call again (nth 0)
    for (int which = 0; which < 3; which++) {
        const char* name = which == 0 ? "fail_select_alloc" : which == 1 ? "fail_public_alloc" : "fail_list_alloc";
        const int last = which == 0 ? 9 : which == 1 ? 7 : 12;
        for (int nth = 1; nth <= last; nth++) {
            OneRow w = make_onerow(host_words, 13, 2, PATH_SETTINGS[0]);
            fheram_bank* b = w.b;
            const fheram_addr* a10[] = {w.a[1], w.a[0]};
            ll::verbose = false;
            fheram_selector* s3 = new_selector(w, 3, 0);
            (void)ll::take_events();
            const fheram_selector* s3s[] = {s3, s3};
            const Src host1[] = {{FHERAM_SRC_HOST, 1}, {FHERAM_SRC_SELECT_RESULT, 0}};
            const fheram_select_lane l2[] = {{FHERAM_SRC_HOST, 1, 0, 0}, {FHERAM_SRC_HOST, 1, 1, 0}};
            const std::string tag = std::string(name) + " " + std::to_string(nth);
            if (which == 0) {
                call(w, tag + ": select_lanes x1 on a fresh bank", [&] { fheram_bank_selftest_fail_select_alloc(b, nth); return fheram_bank_select_lanes(b, s3s, one, 1, l2, w.words.data(), nullptr); });
                call(w, tag + ": select x1, disarmed", [&] { fheram_bank_selftest_fail_select_alloc(b, 0); return fheram_bank_select(b, s3s, one, 1, host1, w.words.data(), nullptr); });
                if (nth <= 7) call(w, tag + ": select x2 grows", [&] { fheram_bank_selftest_fail_select_alloc(b, nth); return fheram_bank_select(b, s3s, two, 2, host1, w.words.data(), nullptr); });
                call(w, tag + ": select x1 of the last select's output, disarmed", [&] { fheram_bank_selftest_fail_select_alloc(b, 0); return fheram_bank_select(b, s3s, one, 1, host1 + 1, nullptr, nullptr); });
            } else if (which == 1) {
                call(w, tag + ": peek on a fresh bank", [&] { fheram_bank_selftest_fail_public_alloc(b, nth); return fheram_bank_peek(b, m10, pa, 2, nullptr); });
                call(w, tag + ": peek, disarmed", [&] { fheram_bank_selftest_fail_public_alloc(b, 0); return fheram_bank_peek(b, m10, pa, 2, nullptr); });
            } else {
                call(w, tag + ": read_prepare_write_list [1, 0] on a fresh bank", [&] { fheram_bank_selftest_fail_list_alloc(b, nth); return fheram_bank_read_prepare_write_list(b, m10, a10, 2, nullptr); });
                call(w, tag + ": read_prepare_write_list [1, 0], disarmed", [&] { fheram_bank_selftest_fail_list_alloc(b, 0); return fheram_bank_read_prepare_write_list(b, m10, a10, 2, nullptr); });
            }
            ll::verbose = false;
            fheram_selector_destroy(s3);
            free_onerow(w);
            ll::verbose = true;
        }
    }
    ll::reserve_mode = false;
}

int onerow_main(long only, unsigned* host_words) {
    ll::path_mode = true; ll::onerow_mode = true;
    std::puts("# arenas: a32=data a33=scrA a34=scrB a35=scrC a36=scrD a37=tree a38=res a39=tmp a40=tmp2 a41=w a42=part a43=trtop; a13=prep a14=prep_inv a27,a28=the encrypted integer a56..=address digits a60=bank prep a61=bank prep_inv;");
    std::puts("# a129.. = device allocations in order (per configuration); p<k> = pinned allocation k (real memory); events: a231.. = created with flags, in order");
    const struct { int lg, ws; const Setting& st; } CONFIGS[] = {{12, 2, PATH_SETTINGS[0]}, {13, 2, PATH_SETTINGS[0]}, {16, 2, PATH_SETTINGS[0]}, {13, 2, PATH_SETTINGS[1]}, {14, 13, PATH_SETTINGS[0]}};
    long id = 0;
    for (const auto& cf : CONFIGS) {
        if (only >= 0 && id != only) { id++; continue; }
        ll::verbose = only >= 0;
        ll::digest = 0xcbf29ce484222325ull; ll::lines = 0; path_ops = 0; ll::n_alloc = 0; ll::n_events = 0;
        std::printf("config %ld: max_addr=2^%d word_size=%d bank of 2 %s\n", id, cf.lg, cf.ws, cf.st.name);
        run_onerow(host_words, cf.lg, cf.ws, cf.st);
        std::printf("config %ld: %" PRIu64 " operations, %" PRIu64 " lines, digest %016" PRIx64 "\n", id, path_ops, ll::lines, ll::digest);
        id++;
    }
    if (only < 0) { ll::verbose = true; run_onerow_refusals(host_words); run_onerow_reserves(host_words); }
    return 0;
}

// ---- config mode: config_in_effect of each input ------------------------------------------------------------------------------------
struct CfgField { const char* name; int32_t fheram_config::*p; };
#define CFG_FIELD(f) {#f, &fheram_config::f}
const CfgField CFG_FIELDS[] = {CFG_FIELD(limb_split), CFG_FIELD(fine_split), CFG_FIELD(memo), CFG_FIELD(pre_inv), CFG_FIELD(tail), CFG_FIELD(tail_test),
                               CFG_FIELD(mid), CFG_FIELD(mid_test), CFG_FIELD(chain), CFG_FIELD(chain_y), CFG_FIELD(pair_z), CFG_FIELD(fuse),
                               CFG_FIELD(graph), CFG_FIELD(safe), CFG_FIELD(nco), CFG_FIELD(tail_ep), CFG_FIELD(monitor)};
const char* const CONFIG_INPUTS[] = {
    "", "memo=0", "memo=0,pre_inv=2", "pre_inv=0", "pre_inv=2", "pre_inv=5", "pre_inv=-1", "graph=1", "graph=1,pre_inv=2", "safe=1", "safe=1,tail_test=2,mid_test=1",
    "safe=1,monitor=0", "safe=1,pre_inv=0", "safe=1,graph=1", "mid=7", "mid=-1", "mid=1", "tail_test=5", "tail_test=-3", "tail=0,tail_test=1", "tail=-1",
    "limb_split=7", "monitor=9", "monitor=-1", "nco=1", "nco=2", "nco=3", "nco=-1", "chain_y=1", "chain_y=0"};
std::string departures(const fheram_config& cfg, const fheram_config* from) {   // from == nullptr: every field
    std::string out;
    for (const CfgField& f : CFG_FIELDS)
        if (!from || cfg.*f.p != from->*f.p) out += (out.empty() ? "" : ", ") + std::string(f.name) + " " + std::to_string(cfg.*f.p);
    return out.empty() ? "D" : out;
}
int config_main() {
    const fheram_config D = config_builtin();
    std::printf("D: %s\n", departures(D, nullptr).c_str());
    for (const char* in : CONFIG_INPUTS) {
        fheram_config asked = D;
        for (const char* q = in; *q; q += std::strcspn(q, ","), q += *q == ',')   // name=value, comma-separated
            for (const CfgField& f : CFG_FIELDS) { const size_t n = std::strlen(f.name); if (!std::strncmp(q, f.name, n) && q[n] == '=') asked.*f.p = std::atoi(q + n + 1); }
        std::printf("%s -> %s\n", in[0] ? in : "(none)", departures(config_in_effect(asked), &D).c_str());
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "config")) return config_main();
    const bool onerow = argc > 1 && !std::strcmp(argv[1], "onerow");
    const bool path = argc > 1 && !std::strcmp(argv[1], "path");
    const long only = argc > 1 + (path || onerow) ? std::atol(argv[1 + (path || onerow)]) : -1;
    unsigned* host_words = static_cast<unsigned*>(mmap(reinterpret_cast<void*>(0x7e0000000000ull), 4096, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_FIXED_NOREPLACE, -1, 0));
    if (host_words == MAP_FAILED) { std::perror("mmap"); return 1; }
    if (onerow) return onerow_main(only, host_words);
    if (path) return path_main(only, host_words);
    long id = 0;
    for (int cus : CUS) for (int s_evk = 4; s_evk <= 5; s_evk++) for (const Setting& st : SETTINGS)
    for (int side = 0; side < 2; side++) for (int graph = 0; graph < 2; graph++) for (int profile = 0; profile < 2; profile++, id++) {
        if (only >= 0 && id != only) continue;
        fheram_ctx* c = make_ctx(host_words);
        c->cus = cus; c->s_evk = s_evk; c->atk = (size_t)fheram_ctx::DNUM_CT * s_evk * 2 * N;
        st.apply(c);
        c->cfg.graph = graph; c->profile = profile;
        c->cur = side ? c->stream2 : c->stream;
        ll::verbose = only >= 0;
        ll::digest = 0xcbf29ce484222325ull; ll::lines = 0;
        const uint64_t c0 = cases;
        std::printf("config %ld: cus=%d s_evk=%d %s side=%d graph=%d profile=%d\n", id, cus, s_evk, st.name, side, graph, profile);
        run_config(c);
        std::printf("config %ld: %" PRIu64 " cases, %" PRIu64 " lines, digest %016" PRIx64 "\n", id, cases - c0, ll::lines, ll::digest);
        delete c;
    }
    std::printf("total: %" PRIu64 " cases\n", cases);
    return 0;
}
