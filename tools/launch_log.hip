// Launch log of the host code's chain dispatch, on the CPU: nothing is launched and no GPU is opened.
//
// hipLaunchKernelGGL is redefined as a recorder of (kernel, grid, workgroup, LDS bytes, stream side, argument bytes); with fake,
// distinct addresses in the context's buffer fields the program calls trace_steps, ep_chain, pack_levels, the row-chain and tail launchers and the predicates path.hpp
// derives from the same decision (Opnds::row_fuse for a context, a batch and a bank range; batch_needs_third; read_top's fuse_ep /
// gated) over a sweep of configurations, chain lengths, grids and buffer layouts.  Two trees dispatch alike exactly when their logs are
// equal, so a change to a launch form is one `diff` away from its evidence:
//
//   hipcc -std=c++17 -O1 --offload-arch=gfx950 -ftrivial-auto-var-init=zero -Wno-unused-variable -I fhe-ram_amd/csrc -I tools -o launch_log tools/launch_log.hip
//   ./launch_log > profiles/chain_form_launch_log.txt      one digest line per configuration (FNV-1a over its launch lines)
//   ./launch_log 17                                        every launch line of configuration 17
//
// -ftrivial-auto-var-init=zero makes the padding of the argument structs part of a reproducible digest.  The include path names the
// csrc/ to log; launch_log_shim.hpp (tools/ for this tree) reaches what has no name of its own there.
// Trace chains are logged for 0 .. LOGN steps (the context has LOGN trace keys), product chains and the predicates for 0 .. CHAIN_MAX + 1.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace ll {
bool verbose = false;
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
template <typename... A>
void record(const char* kernel, const char* site, dim3 g, dim3 b, size_t lds, hipStream_t s, const A&... a) {
    uint64_t h = 0xcbf29ce484222325ull;
    size_t bytes = 0;
    ((h = fnv(h, &a, sizeof(a)), bytes += sizeof(a)), ...);
    char buf[512];
    std::snprintf(buf, sizeof buf, "  %s grid=(%u,%u,%u) wg=%u lds=%zu %s args=%zuB:%016" PRIx64, kernel_name(kernel, site).c_str(), g.x, g.y, g.z, b.x, lds,
                  s == main_stream ? "main" : "side", bytes, h);
    line(buf);
}
}  // namespace ll

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) ll::record(#kernel, __PRETTY_FUNCTION__, grid, block, lds, stream, __VA_ARGS__)
// ProfScope under `profile`: no event is created or recorded
#define hipEventCreate(e) (*(e) = nullptr, hipSuccess)
#define hipEventRecord(e, s) ((void)(e), (void)(s), hipSuccess)

#include "path.hpp"
#include <launch_log_shim.hpp>   // (angle brackets: from the include path, not from beside this file)

namespace {

template <typename P> P fake(int k) { return reinterpret_cast<P>((uintptr_t)0x100000000ull * (uintptr_t)(k + 1)); }
int32_t* arena(int k) { return fake<int32_t*>(32 + k); }

struct Setting { const char* name; void (*apply)(fheram_ctx*); };
const Setting SETTINGS[] = {
    {"default", [](fheram_ctx*) {}},
    {"nco=1", [](fheram_ctx* c) { c->nco = 1; }},
    {"nco=2", [](fheram_ctx* c) { c->nco = 2; }},
    {"limb_split=0", [](fheram_ctx* c) { c->limb_split = 0; }},
    {"fine_split=0", [](fheram_ctx* c) { c->fine_split = 0; }},
    {"tail=0", [](fheram_ctx* c) { c->tail = 0; }},
    {"tail_test=1", [](fheram_ctx* c) { c->tail_test = 1; }},
    {"tail_test=2", [](fheram_ctx* c) { c->tail_test = 2; }},
    {"tail_ep=0", [](fheram_ctx* c) { c->tail_ep = 0; }},
    {"mid=0", [](fheram_ctx* c) { c->mid = 0; }},
    {"mid=1", [](fheram_ctx* c) { c->mid = 1; }},
    {"mid_test=1", [](fheram_ctx* c) { c->mid_test = 1; }},
    {"chain=0", [](fheram_ctx* c) { c->chain = 0; }},
    {"chain_y=0", [](fheram_ctx* c) { c->chain_y = 0; }},
    {"fuse=0", [](fheram_ctx* c) { c->fuse = 0; }},
    {"pair_z=0", [](fheram_ctx* c) { c->pair_z = 0; }},
    {"safe", [](fheram_ctx* c) { c->safe = 1; c->tail = 0; c->tail_test = 0; c->mid = 0; c->mid_test = 0; }},
    {"wide", [](fheram_ctx* c) { c->wide = true; }},
    // the pairs the test suite forces
    {"limb_split=0,nco=1", [](fheram_ctx* c) { c->limb_split = 0; c->nco = 1; }},
    {"limb_split=0,nco=2", [](fheram_ctx* c) { c->limb_split = 0; c->nco = 2; }},
    {"limb_split=0,nco=2,wide", [](fheram_ctx* c) { c->limb_split = 0; c->nco = 2; c->wide = true; }},
    {"limb_split=0,nco=2,chain=0", [](fheram_ctx* c) { c->limb_split = 0; c->nco = 2; c->chain = 0; }},
    {"limb_split=0,nco=2,chain_y=0", [](fheram_ctx* c) { c->limb_split = 0; c->nco = 2; c->chain_y = 0; }},
    {"limb_split=0,nco=2,chain_y=0,wide", [](fheram_ctx* c) { c->limb_split = 0; c->nco = 2; c->chain_y = 0; c->wide = true; }},
    {"limb_split=0,nco=2,fuse=0,pair_z=0", [](fheram_ctx* c) { c->limb_split = 0; c->nco = 2; c->fuse = 0; c->pair_z = 0; }},
    {"chain_y=0,fuse=0,nco=2,limb_split=0", [](fheram_ctx* c) { c->chain_y = 0; c->fuse = 0; c->nco = 2; c->limb_split = 0; }},
    {"mid=0,tail=0", [](fheram_ctx* c) { c->mid = 0; c->tail = 0; }},
    {"tail_ep=0,tail_test=1", [](fheram_ctx* c) { c->tail_ep = 0; c->tail_test = 1; }},
    {"nco=2,mid=0", [](fheram_ctx* c) { c->nco = 2; c->mid = 0; }},
    {"nco=2,fine_split=0", [](fheram_ctx* c) { c->nco = 2; c->fine_split = 0; }},
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
    c->tail = as->tail; c->tail_seq = 0; c->tail_launches = c->tail_launch_mark = 0; c->tail_fb_mark = 0;
    c->mid = as->mid; c->mid_seq = 0; c->mid_launches = c->mid_launch_mark = 0; c->mid_fb_mark = 0; c->mid_bad_windows = c->mid_saved = 0;
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
            const OpndTable t = v ? OpndTable{gy / 2, 1000, gy / 2} : OpndTable{};
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
            const Opnds ctx{c, nullptr, 1, gy, nullptr, nullptr, 0, true}, batch{c, nullptr, 2, (gy + 1) / 2, nullptr, nullptr, 0, false}, bank{c, nullptr, 2, (gy + 1) / 2, nullptr, nullptr, 0, true};
            bits = bits * 8 + (ctx.row_fuse(n, n_tr, gx) ? 1 : 0) + (batch.row_fuse(n, n_tr, gx) ? 2 : 0) + (bank.row_fuse(n, n_tr, gx) ? 4 : 0);
        }
        tail_line("row_fuse (ctx, batch, bank) x n_tr", bits);
        c->rows = (size_t)gx; c->ws = 1; c->base2d[0].assign((size_t)std::max(n, 1), 1);
        bits = 0;
        for (int lg = 0; lg <= LOGN; lg++) { c->rows_glob = (size_t)1 << lg; bits = bits * 2 + (batch_needs_third(c, gy) ? 1 : 0); }
        tail_line("batch_needs_third x log2(rows)", bits);
        tail_line("read_top tail (fuse_ep, gated)", shim_tail_top(c, gx * gy) ? 1 : 0);
        c->rows = c->rows_glob = 1; c->base2d[0].assign(3, 1);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const long only = argc > 1 ? std::atol(argv[1]) : -1;
    unsigned* host_words = static_cast<unsigned*>(mmap(reinterpret_cast<void*>(0x7e0000000000ull), 4096, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_FIXED_NOREPLACE, -1, 0));
    if (host_words == MAP_FAILED) { std::perror("mmap"); return 1; }
    long id = 0;
    for (int cus : CUS) for (int s_evk = 4; s_evk <= 5; s_evk++) for (const Setting& st : SETTINGS)
    for (int side = 0; side < 2; side++) for (int graph = 0; graph < 2; graph++) for (int profile = 0; profile < 2; profile++, id++) {
        if (only >= 0 && id != only) continue;
        fheram_ctx* c = make_ctx(host_words);
        c->cus = cus; c->s_evk = s_evk; c->atk = (size_t)fheram_ctx::DNUM_CT * s_evk * 2 * N;
        st.apply(c);
        c->use_graph = graph; c->profile = profile;
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
