// fheram.hpp — host-side mirror of the reference crate's public interface for the RAM path, in
// C++ (the reference is compiled Rust; this image has no Rust toolchain, see INTEGRATION.md for the
// Rust `extern "C"` binding a maintainer would add).  Header-only, over the C ABI of
// include/fheram.h.  Same names, argument meaning and error behaviour as
//   Parameters              /root/reference/src/parameters.rs:147-287
//   EvaluationKeysPrepared  /root/reference/src/keys.rs:27-71
//   Address                 /root/reference/src/address.rs:21-119
//   Ram                     /root/reference/src/ram.rs:25-294
//   GLWESecret, Source      setup side: the encrypt_sk methods take the caller's samplers (source_xa, source_xe)
// The reference panics on misuse (assert!); these classes throw fheram::Error with the same text.
#pragma once
#include "../../include/fheram.h"

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace fheram {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// GLWE<Vec<u8>> stand-in: int64 limbs in Poulpy's host layout [limb][col][N].
using Glwe = std::vector<int64_t>;

// parameters.rs:147-176
struct Parameters {
    fheram_params p;
    Parameters() { fheram_params_default(&p); }                                   // Parameters::new()
    Parameters(size_t word_size, const std::vector<uint8_t>& decomp_n, size_t max_addr) : Parameters() {   // ram.rs:72-78
        p.word_size = (uint32_t)word_size;
        p.max_addr = max_addr;
        p.n_decomp = (uint32_t)decomp_n.size();
        for (size_t i = 0; i < decomp_n.size() && i < 16; i++) p.decomp_n[i] = decomp_n[i];
    }
    // the block README.md:36's timings were taken with (README.md:20-33): K_GLWE_PT 9, 5-limb trace keys, MAX_ADDR 2^18
    static Parameters readme() {
        Parameters q(4, {4, 4, 4, 4}, (size_t)1 << 18);
        q.p.k_glwe_pt = 9;
        q.p.k_evk_trace = 5 * q.p.base2k;
        return q;
    }
    size_t max_addr() const { return p.max_addr; }            // parameters.rs:237
    size_t word_size() const { return p.word_size; }          // parameters.rs:261
    uint32_t basek() const { return p.base2k; }
    uint32_t rank() const { return p.rank; }
    uint32_t k_glwe_ct() const { return p.k_glwe_ct; }
    uint32_t k_glwe_pt() const { return p.k_glwe_pt; }
    size_t n() const { return (size_t)1 << p.log_n; }
};

// keys.rs:27-31 — std-form keys; `prepare` (keys.rs:57-71) happens on the device at first use.
struct EvaluationKeysPrepared {
    std::vector<int64_t> gal_els;                 // GLWE::trace_galois_elements (keys.rs:39)
    std::vector<std::vector<int64_t>> atk_glwe;   // one GGLWE per Galois element (keys.rs:28)
    std::vector<int64_t> atk_ggsw_inv;            // keys.rs:29, p() must be -1
    std::vector<int64_t> tsk_ggsw_inv;            // keys.rs:30
    int64_t atk_ggsw_inv_p = -1;
};

class Ram;

// What the encrypt_sk methods need from a sampler (Poulpy's `Source` in the reference: source_xa for the
// uniform masks, source_xe for the noise).  Sampling stays on the host; the device does the arithmetic.
struct Source {
    virtual ~Source() = default;
    // `count` uniform limbs in [-2^(base2k-1), 2^(base2k-1))
    virtual void uniform_limbs(int64_t* out, size_t count) = 0;
    // `count` samples of round(N(0, (sigma*scale)^2)), truncated at 6 sigma*scale (Poulpy add_normal)
    virtual void gaussian(int64_t* out, size_t count, double scale) = 0;
};
// noise of a ciphertext at precision k sits on limb ceil(k/base2k)-1, scaled by 2^((limb+1)*base2k - k)
inline double noise_scale(uint32_t k, uint32_t base2k) { return (double)((uint64_t)1 << (((k + base2k - 1) / base2k) * base2k - k)); }

// address.rs:21-24 — the GGSW digits of all coordinates, coordinate-major.
class Address {
public:
    std::vector<std::vector<int64_t>> digits;
    Address() = default;
    explicit Address(std::vector<std::vector<int64_t>> d) : digits(std::move(d)) {}
    ~Address() { if (h_) fheram_address_destroy(h_); }
    Address(const Address&) = delete;
    Address& operator=(const Address&) = delete;

private:
    friend class Ram;
    fheram_addr* h_ = nullptr;
    const void* owner_ = nullptr;
};

// ram.rs:25-29
class Ram {
public:
    Parameters params;
    explicit Ram(int device = 0) : Ram(Parameters(), device) {}                   // Ram::new, ram.rs:59
    Ram(const Parameters& prm, int device = 0) : params(prm) {
        int rc = fheram_ctx_create(&params.p, device, &ctx_);
        if (rc != FHERAM_OK) throw Error(rc, fheram_last_error(nullptr));
    }
    // explicit execution switches (include/fheram.h: fheram_config; start from default_config() and change what differs)
    Ram(const Parameters& prm, const fheram_config& cfg, int device = 0) : params(prm) {
        int rc = fheram_ctx_create_cfg(&params.p, device, 0, 1, &cfg, &ctx_);
        if (rc != FHERAM_OK) throw Error(rc, fheram_last_error(nullptr));
    }
    static fheram_config default_config() { fheram_config c; fheram_config_default(&c); return c; }
    fheram_config config() const {                                                  // the switches in effect
        fheram_config c;
        int rc = fheram_ctx_config(ctx_, &c);
        if (rc != FHERAM_OK) throw Error(rc, "fheram_ctx_config");
        return c;
    }
    static Ram new_from_ram_params(size_t word_size, const std::vector<uint8_t>& decomp_n, size_t max_addr, int device = 0) {   // ram.rs:72
        return Ram(Parameters(word_size, decomp_n, max_addr), device);
    }
    Ram(Ram&& o) noexcept : params(o.params), ctx_(o.ctx_), keys_(o.keys_) { o.ctx_ = nullptr; }
    Ram(const Ram&) = delete;
    ~Ram() { if (ctx_) fheram_ctx_destroy(ctx_); }

    size_t glwe_len() const { return fheram_glwe_len(ctx_); }
    // The exactness contract of the FFT64 arithmetic, checked (include/fheram.h: fheram_roundoff_max): the largest |x - rint(x)| any rounding
    // has seen on this context; throws Error(FHERAM_ERR_PRECISION) once it has passed 3/8, like every call that waits for the device.
    double roundoff_max() {
        double m = 0.0;
        const int rc = fheram_roundoff_max(ctx_, &m);
        if (rc != FHERAM_OK) throw Error(rc, fheram_last_error(ctx_));
        return m;
    }
    void roundoff_reset() { const int rc = fheram_roundoff_reset(ctx_); if (rc != FHERAM_OK) throw Error(rc, fheram_last_error(ctx_)); }

    // Ram::encrypt_sk hand-over (ram.rs:129-167): rows = [word_size][rows][GLWE], already encrypted.
    void load_encrypted(const std::vector<int64_t>& rows) {
        if (rows.size() != params.word_size() * fheram_rows(ctx_) * glwe_len())
            throw Error(FHERAM_ERR_INVALID_ARG, "invalid data: data.len()/ram_chunks != max_addr (ram.rs:150-155)");
        chk(fheram_ram_upload(ctx_, rows.data()));
    }
    // Ram::read, ram.rs:172-191
    std::vector<Glwe> read(Address& address, const EvaluationKeysPrepared& keys) {
        use(keys);
        std::vector<int64_t> out(params.word_size() * glwe_len());
        chk(fheram_read(ctx_, dev(address), out.data()));
        return split(out);
    }
    // addresses.size() independent Ram::read (ram.rs:172-191) of this RAM as one operation (fheram_read_batch, at most
    // FHERAM_READ_BATCH_MAX): result i is what read(*addresses[i], keys) returns
    std::vector<std::vector<Glwe>> read_batch(std::vector<Address*>& addresses, const EvaluationKeysPrepared& keys) {
        if (addresses.empty() || addresses.size() > FHERAM_READ_BATCH_MAX)
            throw Error(FHERAM_ERR_INVALID_ARG, "read_batch takes 1 to FHERAM_READ_BATCH_MAX addresses");
        use(keys);
        std::vector<const fheram_addr*> handles;
        for (Address* a : addresses) {
            if (!a) throw Error(FHERAM_ERR_INVALID_ARG, "null address");
            handles.push_back(dev(*a));
        }
        const size_t one = params.word_size() * glwe_len();
        std::vector<int64_t> out(addresses.size() * one);
        chk(fheram_read_batch(ctx_, handles.data(), (int)handles.size(), out.data()));
        std::vector<std::vector<Glwe>> res;
        for (size_t k = 0; k < addresses.size(); k++) res.push_back(split(std::vector<int64_t>(out.begin() + k * one, out.begin() + (k + 1) * one)));
        return res;
    }
    // Ram::read_prepare_write, ram.rs:196-222
    std::vector<Glwe> read_prepare_write(Address& address, const EvaluationKeysPrepared& keys) {
        use(keys);
        std::vector<int64_t> out(params.word_size() * glwe_len());
        chk(fheram_read_prepare_write(ctx_, dev(address), out.data()));
        return split(out);
    }
    // Ram::write, ram.rs:226-294.  Each w[i] must encrypt [w,0,...,0] (ram.rs:228).
    void write(const std::vector<Glwe>& w, Address& address, const EvaluationKeysPrepared& keys) {
        use(keys);
        std::vector<int64_t> flat;
        for (auto& g : w) flat.insert(flat.end(), g.begin(), g.end());
        chk(fheram_write(ctx_, flat.data(), (int)w.size(), dev(address)));
    }
    bool state() const { return fheram_ram_state(ctx_) != 0; }                    // SubRam::state, ram.rs:302
    // Health of the single-launch chains (in-kernel hand-offs): how many were launched and how many gave up and were redone by
    // the launch behind them (0 on a GPU this context has to itself; INTEGRATION.md, "Sharing a GPU")
    struct ChainStats { uint64_t launches = 0, redone = 0; };
    ChainStats tail_stats() { ChainStats s; chk(fheram_tail_stats(ctx_, &s.launches, &s.redone)); return s; }
    ChainStats mid_stats() { ChainStats s; chk(fheram_mid_stats(ctx_, &s.launches, &s.redone)); return s; }
    // The result of the last read / read_prepare_write where the device left it: [word_size][GLWE] int64 in the context's
    // pinned host buffer (no copy on the host); valid until the next operation on this Ram.
    const int64_t* result_view() {
        const int64_t* v = nullptr;
        chk(fheram_result_map(ctx_, &v));
        return v;
    }

    // ---- setup side on the device (include/fheram.h, "Setup side on the device") -------------------
    // GLWESecret + GLWESecretPrepared, examples/fhe-ram.rs:49-59
    class Secret {
    public:
        Secret(Ram& ram, const std::vector<int64_t>& sk) : ram_(ram) { ram.chk(fheram_secret_create(ram.ctx_, sk.data(), &h_)); }
        ~Secret() { if (h_) fheram_secret_destroy(h_); }
        Secret(const Secret&) = delete;
    private:
        friend class Ram;
        Ram& ram_;
        fheram_secret* h_ = nullptr;
    };
    // Ram::encrypt_sk, ram.rs:129-167
    void encrypt_sk(const std::vector<uint8_t>& data, const Secret& sk, Source& source_xa, Source& source_xe) {
        const size_t n = params.n(), glwes = params.word_size() * fheram_rows(ctx_);
        const size_t size = (params.k_glwe_ct() + params.basek() - 1) / params.basek();
        std::vector<int64_t> mask(glwes * size * n), noise(glwes * n);
        source_xa.uniform_limbs(mask.data(), mask.size());
        source_xe.gaussian(noise.data(), noise.size(), noise_scale(params.k_glwe_ct(), params.basek()));
        chk(fheram_ram_encrypt_sk(ctx_, sk.h_, data.data(), data.size(), mask.data(), noise.data()));
    }
    // Address::encrypt_sk, address.rs:86-109: the digits are created on the device
    void encrypt_address(Address& a, uint32_t value, const Secret& sk, Source& source_xa, Source& source_xe) {
        const size_t n = params.n(), size = (params.p.k_ggsw_addr + params.basek() - 1) / params.basek();
        const size_t glwes = (size_t)fheram_n_digits(ctx_) * ((params.k_glwe_ct() + params.basek() - 1) / params.basek()) * 2;   // dnum_ct rows x 2
        std::vector<int64_t> mask(glwes * size * n), noise(glwes * n);
        source_xa.uniform_limbs(mask.data(), mask.size());
        source_xe.gaussian(noise.data(), noise.size(), noise_scale(params.p.k_ggsw_addr, params.basek()));
        if (a.h_) { fheram_address_destroy(a.h_); a.h_ = nullptr; }
        chk(fheram_address_encrypt_sk(ctx_, sk.h_, value, mask.data(), noise.data(), &a.h_));
        a.owner_ = this;
    }
    // poulpy-schemes' FheUintPrepared<u32> as the path needs it (conversion.rs:68-82): one GGSW per bit, on this device
    class FheUintPrepared {
    public:
        // FheUintPrepared::encrypt_sk (conversion.rs:160-168) with the caller's samplers
        FheUintPrepared(Ram& ram, uint32_t value, const Secret& sk, Source& source_xa, Source& source_xe, int n_bits = 32) {
            const size_t n = ram.params.n(), b = ram.params.basek(), k = ram.params.p.k_evk_ggsw_inv;
            const size_t size = (k + b - 1) / b, dnum = (ram.params.p.k_ggsw_addr + b - 1) / b, glwes = (size_t)n_bits * dnum * 2;
            std::vector<int64_t> mask(glwes * size * n), noise(glwes * n);
            source_xa.uniform_limbs(mask.data(), mask.size());
            source_xe.gaussian(noise.data(), noise.size(), noise_scale((uint32_t)k, (uint32_t)b));
            ram.chk(fheram_fheuint_encrypt_sk(ram.ctx_, sk.h_, value, n_bits, mask.data(), noise.data(), &h_));
        }
        // from host ciphertexts: [n_bits][fheram_fheuint_ggsw_len]
        FheUintPrepared(Ram& ram, const std::vector<int64_t>& bits, int n_bits) { ram.chk(fheram_fheuint_create(ram.ctx_, bits.data(), n_bits, &h_)); }
        ~FheUintPrepared() { if (h_) fheram_fheuint_destroy(h_); }
        FheUintPrepared(const FheUintPrepared&) = delete;
    private:
        friend class Ram;
        fheram_fheuint* h_ = nullptr;
    };
    // Address::set_from_fheuint, conversion.rs:68-82 (sign = false: the convention of Address::encrypt_sk, i.e. an
    // address Ram::read accepts; true: what the reference's test decrypts to)
    void set_from_fheuint(Address& a, const FheUintPrepared& fheuint, bool sign = false) {
        if (a.h_) { fheram_address_destroy(a.h_); a.h_ = nullptr; }
        chk(fheram_address_set_from_fheuint(ctx_, fheuint.h_, sign ? 1 : 0, &a.h_));
        a.owner_ = this;
    }
    // The same for 1 to FHERAM_DERIVE_MAX integers as ONE launch on this Ram's stream (fheram_address_derive): no allocation, no host wait;
    // later operations that use the addresses are ordered behind it.  *addrs[i] is overwritten in place when it already lives on this
    // Ram's device (whatever made it) and gets its device buffers here otherwise; its host digits are dropped.  No address twice.  The
    // integers must stay alive until sync().  first_bits (one per integer, or none): the address bits start at bit first_bits[i] of integer i
    // (fheram_address_derive_at: a byte address keeps its lane offset below its word address), one launch per distinct first bit.
    void derive(const std::vector<const FheUintPrepared*>& fheuints, const std::vector<Address*>& addrs, bool sign = false, const std::vector<int>& first_bits = {}) {
        if (fheuints.empty() || fheuints.size() > FHERAM_DERIVE_MAX || addrs.size() != fheuints.size() || (!first_bits.empty() && first_bits.size() != fheuints.size()))
            throw Error(FHERAM_ERR_INVALID_ARG, "derive takes 1 to FHERAM_DERIVE_MAX integers, as many addresses and no or as many first bits");
        std::vector<const fheram_fheuint*> fh;
        std::vector<fheram_addr*> ah;
        for (const FheUintPrepared* f : fheuints) { if (!f) throw Error(FHERAM_ERR_INVALID_ARG, "null integer"); fh.push_back(f->h_); }
        for (Address* a : addrs) {
            if (!a) throw Error(FHERAM_ERR_INVALID_ARG, "null address");
            if (a->h_ && a->owner_ != this) { fheram_address_destroy(a->h_); a->h_ = nullptr; }
            if (!a->h_) { chk(fheram_address_alloc(ctx_, &a->h_)); a->owner_ = this; }
            ah.push_back(a->h_);
        }
        if (first_bits.empty()) chk(fheram_address_derive(ctx_, fh.data(), (int)fh.size(), sign ? 1 : 0, ah.data()));
        else chk(fheram_address_derive_at(ctx_, fh.data(), first_bits.data(), (int)fh.size(), sign ? 1 : 0, ah.data()));
        for (Address* a : addrs) a->digits.clear();
    }
    // EvaluationKeys::encrypt_sk + EvaluationKeysPrepared::prepare, keys.rs:135-180,57-71: generated and
    // prepared on this context; `keys` is marked as the set in use (its std forms stay empty).
    void encrypt_keys(EvaluationKeysPrepared& keys, const Secret& sk, Source& source_xa, Source& source_xe) {
        const size_t n = params.n(), b = params.basek();
        const size_t s4 = (params.p.k_evk_trace + b - 1) / b, s5 = (params.p.k_evk_ggsw_inv + b - 1) / b;
        const size_t dnum_ct = (params.k_glwe_ct() + b - 1) / b, dnum_ggsw = (params.p.k_ggsw_addr + b - 1) / b;   // parameters.rs:273-279
        const size_t n4 = params.p.log_n * dnum_ct, n5 = 2 * dnum_ggsw;
        std::vector<int64_t> mask((n4 * s4 + n5 * s5) * n), noise((n4 + n5) * n);
        source_xa.uniform_limbs(mask.data(), n4 * s4 * n);
        source_xa.uniform_limbs(mask.data() + n4 * s4 * n, n5 * s5 * n);
        source_xe.gaussian(noise.data(), n4 * n, noise_scale(params.p.k_evk_trace, params.basek()));
        source_xe.gaussian(noise.data() + n4 * n, n5 * n, noise_scale(params.p.k_evk_ggsw_inv, params.basek()));
        chk(fheram_keys_encrypt_sk(ctx_, sk.h_, mask.data(), noise.data(), nullptr));
        keys_ = &keys;
    }
    // GLWE::decrypt (examples/fhe-ram.rs:217-222): normalised plaintext limbs [n][size][N]
    std::vector<int64_t> decrypt(const std::vector<Glwe>& cts, const Secret& sk) {
        std::vector<int64_t> flat, pt(cts.size() * glwe_len() / 2);
        for (auto& g : cts) flat.insert(flat.end(), g.begin(), g.end());
        chk(fheram_glwe_decrypt(ctx_, sk.h_, (int)cts.size(), (int)(glwe_len() / (2 * params.n())), flat.data(), pt.data()));
        return pt;
    }

private:
    fheram_ctx* ctx_ = nullptr;
    const EvaluationKeysPrepared* keys_ = nullptr;
    void chk(int rc) { if (rc != FHERAM_OK) throw Error(rc, fheram_last_error(ctx_)); }
    void use(const EvaluationKeysPrepared& k) {
        if (keys_ == &k) return;
        std::vector<const int64_t*> ptr;
        for (auto& a : k.atk_glwe) ptr.push_back(a.data());
        chk(fheram_keys_load(ctx_, k.gal_els.data(), (int)k.gal_els.size(), ptr.data(), k.atk_ggsw_inv.data(), k.atk_ggsw_inv_p,
                             k.tsk_ggsw_inv.data()));
        keys_ = &k;
    }
    fheram_addr* dev(Address& a) {
        if (a.h_ && a.owner_ == this) return a.h_;
        if (a.h_) { fheram_address_destroy(a.h_); a.h_ = nullptr; }
        std::vector<const int64_t*> ptr;
        for (auto& d : a.digits) ptr.push_back(d.data());
        chk(fheram_address_create(ctx_, ptr.data(), (int)ptr.size(), &a.h_));     // layout check of ram.rs:404
        a.owner_ = this;
        return a.h_;
    }
    std::vector<Glwe> split(const std::vector<int64_t>& flat) const {
        std::vector<Glwe> out;
        const size_t g = glwe_len();
        for (size_t i = 0; i < params.word_size(); i++) out.emplace_back(flat.begin() + i * g, flat.begin() + (i + 1) * g);
        return out;
    }
};

// Ram (ram.rs:25-29) over several GPUs of one node behind ONE handle: the native row-sharded path (fheram_group_*) for a
// single-process host.  Same three calls, one per op; `devices` a power of two of HIP device indices.
class GroupRam {
public:
    Parameters params;
    GroupRam(const Parameters& prm, const std::vector<int>& devices) : params(prm) {
        int rc = fheram_group_create(&params.p, devices.data(), (int)devices.size(), &grp_);
        if (rc != FHERAM_OK) throw Error(rc, fheram_group_last_error(nullptr));
    }
    GroupRam(const GroupRam&) = delete;
    ~GroupRam() {
        for (auto& kv : addr_) fheram_group_address_destroy(kv.second);
        if (grp_) fheram_group_destroy(grp_);
    }
    int size() const { return fheram_group_size(grp_); }
    size_t glwe_len() const { return fheram_glwe_len(fheram_group_ctx(grp_, 0)); }
    // the whole RAM [word_size][rows][GLWE] (Ram::encrypt_sk output, ram.rs:129-167); scattered by shard
    void load_encrypted(const std::vector<int64_t>& rows) { chk(fheram_group_ram_upload(grp_, rows.data())); }
    std::vector<Glwe> read(Address& address, const EvaluationKeysPrepared& keys) {                   // ram.rs:172-191
        use(keys);
        std::vector<int64_t> out(params.word_size() * glwe_len());
        chk(fheram_group_read(grp_, dev(address), out.data()));
        return split(out);
    }
    std::vector<Glwe> read_prepare_write(Address& address, const EvaluationKeysPrepared& keys) {     // ram.rs:196-222
        use(keys);
        std::vector<int64_t> out(params.word_size() * glwe_len());
        chk(fheram_group_read_prepare_write(grp_, dev(address), out.data()));
        return split(out);
    }
    void write(const std::vector<Glwe>& w, Address& address, const EvaluationKeysPrepared& keys) {   // ram.rs:226-294
        use(keys);
        std::vector<int64_t> flat;
        for (auto& g : w) flat.insert(flat.end(), g.begin(), g.end());
        chk(fheram_group_write(grp_, flat.data(), (int)w.size(), dev(address)));
    }
    bool state() const { return fheram_group_ram_state(grp_) != 0; }

private:
    fheram_group* grp_ = nullptr;
    const EvaluationKeysPrepared* keys_ = nullptr;
    std::vector<std::pair<const Address*, fheram_group_addr*>> addr_;   // replicated device copies, by host address object
    void chk(int rc) { if (rc != FHERAM_OK) throw Error(rc, fheram_group_last_error(grp_)); }
    void use(const EvaluationKeysPrepared& k) {
        if (keys_ == &k) return;
        std::vector<const int64_t*> ptr;
        for (auto& a : k.atk_glwe) ptr.push_back(a.data());
        chk(fheram_group_keys_load(grp_, k.gal_els.data(), (int)k.gal_els.size(), ptr.data(), k.atk_ggsw_inv.data(), k.atk_ggsw_inv_p,
                                   k.tsk_ggsw_inv.data()));
        keys_ = &k;
    }
    fheram_group_addr* dev(const Address& a) {
        for (auto& kv : addr_) if (kv.first == &a) return kv.second;
        std::vector<const int64_t*> ptr;
        for (auto& d : a.digits) ptr.push_back(d.data());
        fheram_group_addr* h = nullptr;
        chk(fheram_group_address_create(grp_, ptr.data(), (int)ptr.size(), &h));
        addr_.emplace_back(&a, h);
        return h;
    }
    std::vector<Glwe> split(const std::vector<int64_t>& flat) const {
        std::vector<Glwe> out;
        const size_t g = glwe_len();
        for (size_t i = 0; i < params.word_size(); i++) out.emplace_back(flat.begin() + i * g, flat.begin() + (i + 1) * g);
        return out;
    }
};

// M RAMs (ram.rs:25-29) of the same shape under ONE prepared key set on one GPU (fheram_bank_*): read / read_prepare_write / write on
// the contiguous member range [first, first + addresses.size()) as ONE operation, one address per member.  Member m behaves exactly
// like a Ram driven through the same calls; members outside a range are untouched; a refused call changes no member.
class Bank {
public:
    Parameters params;
    Bank(const Parameters& prm, int n_members, int device = 0) : params(prm) {
        int rc = fheram_bank_create(&params.p, device, n_members, nullptr, &bank_);
        if (rc != FHERAM_OK) throw Error(rc, fheram_bank_last_error(nullptr));
    }
    Bank(const Parameters& prm, int n_members, const fheram_config& cfg, int device = 0) : params(prm) {
        int rc = fheram_bank_create(&params.p, device, n_members, &cfg, &bank_);
        if (rc != FHERAM_OK) throw Error(rc, fheram_bank_last_error(nullptr));
    }
    Bank(const Bank&) = delete;
    ~Bank() {
        for (auto& kv : addr_) fheram_address_destroy(kv.second);
        if (bank_) fheram_bank_destroy(bank_);
    }
    int size() const { return fheram_bank_size(bank_); }
    size_t glwe_len() const { return ((params.k_glwe_ct() + params.basek() - 1) / params.basek()) * 2 * params.n(); }
    // one member's rows [word_size][rows][GLWE] (Ram::encrypt_sk output, ram.rs:129-167); the member becomes readable
    void load_encrypted(int member, const std::vector<int64_t>& rows) {
        if (rows.size() != params.word_size() * ((params.max_addr() + params.n() - 1) / params.n()) * glwe_len())
            throw Error(FHERAM_ERR_INVALID_ARG, "invalid data: data.len()/ram_chunks != max_addr (ram.rs:150-155)");
        chk(fheram_bank_ram_upload(bank_, member, rows.data()));
    }
    std::vector<int64_t> store_encrypted(int member) {
        std::vector<int64_t> rows(params.word_size() * ((params.max_addr() + params.n() - 1) / params.n()) * glwe_len());
        chk(fheram_bank_ram_download(bank_, member, rows.data()));
        return rows;
    }
    bool state(int member) const { return fheram_bank_ram_state(bank_, member) != 0; }            // SubRam::state, ram.rs:302
    // result k = what member first + k's Ram::read(*addresses[k]) returns (ram.rs:172-191)
    std::vector<std::vector<Glwe>> read(std::vector<Address*>& addresses, const EvaluationKeysPrepared& keys, int first = 0) {
        return read_op(false, addresses, keys, first);
    }
    std::vector<std::vector<Glwe>> read_prepare_write(std::vector<Address*>& addresses, const EvaluationKeysPrepared& keys, int first = 0) {   // ram.rs:196-222
        return read_op(true, addresses, keys, first);
    }
    // members.size() independent reads as ONE operation (fheram_bank_read_list), entry k on member members[k] at *addresses[k]: any order,
    // any repetition, any subset of the members; 1 to FHERAM_READ_LIST_MAX entries and entries * word_size <= 64.  Result k is what
    // read({addresses[k]}, keys, members[k]) returns, and the bank is left where that sequence of single-member reads leaves it.
    std::vector<std::vector<Glwe>> read_list(const std::vector<int>& members, std::vector<Address*>& addresses, const EvaluationKeysPrepared& keys) {
        if (members.empty() || members.size() > FHERAM_READ_LIST_MAX || addresses.size() != members.size())
            throw Error(FHERAM_ERR_INVALID_ARG, "read_list takes 1 to FHERAM_READ_LIST_MAX members and as many addresses");
        use(keys);
        std::vector<const fheram_addr*> h = handles(addresses);
        std::vector<int64_t> out(h.size() * params.word_size() * glwe_len());
        chk(fheram_bank_read_list(bank_, members.data(), h.data(), (int)h.size(), out.data()));
        return split(out, h.size());
    }
    // entries [first, first + n) of the last list (fheram_bank_read_list_result)
    std::vector<std::vector<Glwe>> list_result(int first, int n) {
        if (n < 1) throw Error(FHERAM_ERR_INVALID_ARG, "empty slice of the last list");
        std::vector<int64_t> out((size_t)n * params.word_size() * glwe_len());
        chk(fheram_bank_read_list_result(bank_, first, n, out.data()));
        return split(out, (size_t)n);
    }
    // w[k]: the word_size GLWEs of member first + k (ram.rs:226-294)
    void write(const std::vector<std::vector<Glwe>>& w, std::vector<Address*>& addresses, const EvaluationKeysPrepared& keys, int first = 0) {
        if (w.size() != addresses.size()) throw Error(FHERAM_ERR_INVALID_ARG, "one word per address");
        std::vector<int64_t> flat;
        for (auto& word : w) {
            if (word.size() != params.word_size()) throw Error(FHERAM_ERR_INVALID_ARG, "w.len() != subrams.len() (ram.rs:243)");
            for (auto& g : word) flat.insert(flat.end(), g.begin(), g.end());
        }
        use(keys);
        std::vector<const fheram_addr*> h = handles(addresses);
        chk(fheram_bank_write(bank_, first, (int)h.size(), flat.data(), h.data()));
    }
    // read_prepare_write of ANY set of members as ONE operation (fheram_bank_read_prepare_write_list), entry k on member members[k] at
    // *addresses[k]: distinct members (a RAM has one pending write), any order, any subset.  Result k is what
    // read_prepare_write({addresses[k]}, keys, members[k]) returns; every named member is then prepared like any other.
    std::vector<std::vector<Glwe>> read_prepare_write_list(const std::vector<int>& members, std::vector<Address*>& addresses, const EvaluationKeysPrepared& keys) {
        if (members.empty() || addresses.size() != members.size())
            throw Error(FHERAM_ERR_INVALID_ARG, "read_prepare_write_list takes at least one member and as many addresses");
        use(keys);
        std::vector<const fheram_addr*> h = handles(addresses);
        std::vector<int64_t> out(h.size() * params.word_size() * glwe_len());
        chk(fheram_bank_read_prepare_write_list(bank_, members.data(), h.data(), (int)h.size(), out.data()));
        return split(out, h.size());
    }
    // w[k]: the word_size GLWEs written to member members[k] at *addresses[k] (fheram_bank_write_list); the members are in state 1,
    // however they were prepared (a list, a range, single calls)
    void write_list(const std::vector<int>& members, const std::vector<std::vector<Glwe>>& w, std::vector<Address*>& addresses, const EvaluationKeysPrepared& keys) {
        if (members.empty() || addresses.size() != members.size() || w.size() != members.size())
            throw Error(FHERAM_ERR_INVALID_ARG, "write_list takes at least one member, as many addresses and one word per member");
        std::vector<int64_t> flat;
        for (auto& word : w) {
            if (word.size() != params.word_size()) throw Error(FHERAM_ERR_INVALID_ARG, "w.len() != subrams.len() (ram.rs:243)");
            for (auto& g : word) flat.insert(flat.end(), g.begin(), g.end());
        }
        use(keys);
        std::vector<const fheram_addr*> h = handles(addresses);
        chk(fheram_bank_write_list(bank_, members.data(), h.data(), (int)h.size(), flat.data()));
    }
    // ---- the setup side of a bank (include/fheram.h, "Setup side of a bank"): what Ram's setup side is to a context.  Sampling stays on the
    // host (Source); every call waits for the device.
    // GLWESecret + GLWESecretPrepared on the bank's device (fheram_bank_secret_create); the bank or the secret may go first
    class Secret {
    public:
        Secret(Bank& bank, const std::vector<int64_t>& sk) { bank.chk(fheram_bank_secret_create(bank.bank_, sk.data(), &h_)); }
        ~Secret() { if (h_) fheram_secret_destroy(h_); }
        Secret(const Secret&) = delete;
    private:
        friend class Bank;
        fheram_secret* h_ = nullptr;
    };
    // an encrypted integer on the bank's device, from host ciphertexts [n_bits][fheram_fheuint_ggsw_len] (fheram_bank_fheuint_create)
    class FheUintPrepared {
    public:
        FheUintPrepared(Bank& bank, const std::vector<int64_t>& bits, int n_bits) { bank.chk(fheram_bank_fheuint_create(bank.bank_, bits.data(), n_bits, &h_)); }
        // FheUintPrepared::encrypt_sk (conversion.rs:160-168) with the caller's samplers (fheram_bank_fheuint_encrypt_sk)
        FheUintPrepared(Bank& bank, uint32_t value, const Secret& sk, Source& source_xa, Source& source_xe, int n_bits = 32) {
            const size_t n = bank.params.n(), b = bank.params.basek(), k = bank.params.p.k_evk_ggsw_inv;
            const size_t size = (k + b - 1) / b, dnum = (bank.params.p.k_ggsw_addr + b - 1) / b, glwes = (size_t)n_bits * dnum * 2;
            std::vector<int64_t> mask(glwes * size * n), noise(glwes * n);
            source_xa.uniform_limbs(mask.data(), mask.size());
            source_xe.gaussian(noise.data(), noise.size(), noise_scale((uint32_t)k, (uint32_t)b));
            bank.chk(fheram_bank_fheuint_encrypt_sk(bank.bank_, sk.h_, value, n_bits, mask.data(), noise.data(), &h_));
        }
        ~FheUintPrepared() { if (h_) fheram_fheuint_destroy(h_); }
        FheUintPrepared(const FheUintPrepared&) = delete;
    private:
        friend class Bank;
        fheram_fheuint* h_ = nullptr;
    };
    // as Ram::derive (fheram_bank_address_derive / _derive_at): *addrs[i] becomes an ordinary address of this bank, which may serve several members
    void derive(const std::vector<const FheUintPrepared*>& fheuints, const std::vector<Address*>& addrs, bool sign = false, const std::vector<int>& first_bits = {}) {
        if (fheuints.empty() || fheuints.size() > FHERAM_DERIVE_MAX || addrs.size() != fheuints.size() || (!first_bits.empty() && first_bits.size() != fheuints.size()))
            throw Error(FHERAM_ERR_INVALID_ARG, "derive takes 1 to FHERAM_DERIVE_MAX integers, as many addresses and no or as many first bits");
        std::vector<const fheram_fheuint*> fh;
        std::vector<fheram_addr*> ah;
        for (const FheUintPrepared* f : fheuints) { if (!f) throw Error(FHERAM_ERR_INVALID_ARG, "null integer"); fh.push_back(f->h_); }
        for (Address* a : addrs) {
            if (!a) throw Error(FHERAM_ERR_INVALID_ARG, "null address");
            fheram_addr* h = nullptr;
            for (auto& kv : addr_) if (kv.first == a) h = kv.second;
            if (!h) { chk(fheram_bank_address_alloc(bank_, &h)); addr_.emplace_back(a, h); }
            ah.push_back(h);
        }
        if (first_bits.empty()) chk(fheram_bank_address_derive(bank_, fh.data(), (int)fh.size(), sign ? 1 : 0, ah.data()));
        else chk(fheram_bank_address_derive_at(bank_, fh.data(), first_bits.data(), (int)fh.size(), sign ? 1 : 0, ah.data()));
        for (Address* a : addrs) a->digits.clear();
    }
    // ---- oblivious select (include/fheram.h): pick one of the candidate words by an encrypted index, on the device
    // the encrypted index over up to 2^bits candidates: from host std-form GGSW digits (fheram_bank_selector_create), or without digits, for derive_selectors
    class RegFile;
    class Selector {
    public:
        Selector(Bank& bank, int bits) { bank.chk(fheram_bank_selector_alloc(bank.bank_, bits, &h_)); }
        Selector(Bank& bank, int bits, const std::vector<std::vector<int64_t>>& digits) {
            std::vector<const int64_t*> ptr;
            for (auto& d : digits) ptr.push_back(d.data());
            bank.chk(fheram_bank_selector_create(bank.bank_, ptr.data(), (int)ptr.size(), bits, &h_));
        }
        // a FIELD selector: digit d has widths[d] bits and may come from an integer and a bit position of its own (fheram_bank_selector_alloc_fields /
        // _create_fields); without digits for derive_selector_fields, or from host std-form GGSW digits, one per field
        Selector(Bank& bank, const std::vector<int>& widths) : fields_(widths.size()) { bank.chk(fheram_bank_selector_alloc_fields(bank.bank_, widths.data(), (int)widths.size(), &h_)); }
        Selector(Bank& bank, const std::vector<int>& widths, const std::vector<std::vector<int64_t>>& digits) : fields_(widths.size()) {
            std::vector<const int64_t*> ptr;
            for (auto& d : digits) ptr.push_back(d.data());
            bank.chk(fheram_bank_selector_create_fields(bank.bank_, ptr.data(), (int)ptr.size(), widths.data(), (int)widths.size(), &h_));
        }
        // a WIDE selector, the address of a Table: up to FHERAM_TABLE_BITS_MAX bits (fheram_bank_table_selector_alloc / _create / _alloc_fields)
        struct Wide {};
        Selector(Bank& bank, Wide, int bits) { bank.chk(fheram_bank_table_selector_alloc(bank.bank_, bits, &h_)); }
        Selector(Bank& bank, Wide, int bits, const std::vector<std::vector<int64_t>>& digits) {
            std::vector<const int64_t*> ptr;
            for (auto& d : digits) ptr.push_back(d.data());
            bank.chk(fheram_bank_table_selector_create(bank.bank_, ptr.data(), (int)ptr.size(), bits, &h_));
        }
        Selector(Bank& bank, Wide, const std::vector<int>& widths) : fields_(widths.size()) { bank.chk(fheram_bank_table_selector_alloc_fields(bank.bank_, widths.data(), (int)widths.size(), &h_)); }
        ~Selector() { if (h_) fheram_selector_destroy(h_); }
        Selector(const Selector&) = delete;
        int n_digits() const { return fheram_selector_n_digits(h_); }
        // fills the selector, in place, with Address::encrypt_sk's digits of `value` over its own plan (fheram_bank_selector_encrypt_sk)
        void encrypt_sk(Bank& bank, uint32_t value, const Secret& sk, Source& source_xa, Source& source_xe) {
            const size_t n = bank.params.n(), b = bank.params.basek(), size = (bank.params.p.k_ggsw_addr + b - 1) / b;
            const size_t glwes = (size_t)n_digits() * ((bank.params.k_glwe_ct() + b - 1) / b) * 2;   // dnum_ct rows x 2
            std::vector<int64_t> mask(glwes * size * n), noise(glwes * n);
            source_xa.uniform_limbs(mask.data(), mask.size());
            source_xe.gaussian(noise.data(), noise.size(), noise_scale(bank.params.p.k_ggsw_addr, (uint32_t)b));
            bank.chk(fheram_bank_selector_encrypt_sk(bank.bank_, sk.h_, h_, value, mask.data(), noise.data()));
        }
    private:
        friend class Bank;
        friend class RegFile;
        fheram_selector* h_ = nullptr;
        size_t fields_ = 0;   // a field selector: its number of fields
    };
    // digit d of the field selector <- bits [first_bits[d], first_bits[d] + widths[d]) of *fheuints[d] (fheram_bank_selector_derive_fields)
    void derive_selector_fields(Selector& sel, const std::vector<const FheUintPrepared*>& fheuints, const std::vector<int>& first_bits) {
        if (!sel.fields_ || fheuints.size() != sel.fields_ || first_bits.size() != sel.fields_)
            throw Error(FHERAM_ERR_INVALID_ARG, "derive_selector_fields takes a field selector and one integer and one first bit per field");
        std::vector<const fheram_fheuint*> fh;
        for (const FheUintPrepared* f : fheuints) { if (!f) throw Error(FHERAM_ERR_INVALID_ARG, "null integer"); fh.push_back(f->h_); }
        chk(fheram_bank_selector_derive_fields(bank_, sel.h_, fh.data(), first_bits.data()));
    }
    // *sels[i] <- bits [first_bits[i], first_bits[i] + bits_i) of *fheuints[i] (fheram_bank_selector_derive): no allocation, no host wait
    void derive_selectors(const std::vector<const FheUintPrepared*>& fheuints, const std::vector<int>& first_bits, const std::vector<Selector*>& sels) {
        if (sels.empty() || sels.size() > FHERAM_SELECT_MAX || fheuints.size() != sels.size() || first_bits.size() != sels.size())
            throw Error(FHERAM_ERR_INVALID_ARG, "derive_selectors takes 1 to FHERAM_SELECT_MAX selectors and as many integers and first bits");
        std::vector<const fheram_fheuint*> fh;
        std::vector<fheram_selector*> sh;
        for (const FheUintPrepared* f : fheuints) { if (!f) throw Error(FHERAM_ERR_INVALID_ARG, "null integer"); fh.push_back(f->h_); }
        for (Selector* x : sels) { if (!x) throw Error(FHERAM_ERR_INVALID_ARG, "null selector"); sh.push_back(x->h_); }
        chk(fheram_bank_selector_derive(bank_, fh.data(), first_bits.data(), (int)sh.size(), sh.data()));
    }
    // ---- the derive list (fheram_bank_derive_list): any mix of addresses, selectors and selector fields from encrypted integers as ONE launch
    struct DeriveItem { int kind; const FheUintPrepared* fu; Address* addr; Selector* sel; int first_bit; bool sign; int field; };
    // *addr <- the address read from bits [first_bit, ..) of fu
    static DeriveItem derive_address(const FheUintPrepared& fu, Address& addr, int first_bit = 0, bool sign = false) { return {FHERAM_DERIVE_ADDRESS, &fu, &addr, nullptr, first_bit, sign, 0}; }
    // the plain selector sel <- bits [first_bit, first_bit + bits) of fu
    static DeriveItem derive_selector(const FheUintPrepared& fu, Selector& sel, int first_bit = 0) { return {FHERAM_DERIVE_SELECTOR, &fu, nullptr, &sel, first_bit, false, 0}; }
    // digit `field` of the field selector sel <- bits [first_bit, first_bit + widths[field]) of fu; a call names every field of such a selector
    static DeriveItem derive_field(const FheUintPrepared& fu, Selector& sel, int field, int first_bit = 0) { return {FHERAM_DERIVE_FIELD, &fu, nullptr, &sel, first_bit, false, field}; }
    void derive_list(const std::vector<DeriveItem>& items) {
        if (items.empty() || items.size() > FHERAM_DERIVE_LIST_MAX) throw Error(FHERAM_ERR_INVALID_ARG, "derive_list takes 1 to FHERAM_DERIVE_LIST_MAX items");
        std::vector<fheram_derive_item> ci;
        for (const DeriveItem& it : items) {
            if (!it.fu || (it.kind == FHERAM_DERIVE_ADDRESS ? !it.addr : !it.sel)) throw Error(FHERAM_ERR_INVALID_ARG, "a derive item without its integer or target");
            void* target = it.kind == FHERAM_DERIVE_ADDRESS ? nullptr : (void*)it.sel->h_;
            if (it.kind == FHERAM_DERIVE_ADDRESS) {
                fheram_addr* h = nullptr;
                for (auto& kv : addr_) if (kv.first == it.addr) h = kv.second;
                if (!h) { chk(fheram_bank_address_alloc(bank_, &h)); addr_.emplace_back(it.addr, h); }
                target = h;
            }
            ci.push_back(fheram_derive_item{it.kind, it.first_bit, it.sign ? 1 : 0, it.field, it.fu->h_, target});
        }
        chk(fheram_bank_derive_list(bank_, ci.data(), (int)ci.size()));
        for (const DeriveItem& it : items) if (it.kind == FHERAM_DERIVE_ADDRESS) it.addr->digits.clear();
    }
    // the digits of an address of this bank: get_base_2d's count (base.rs:84-108) on the parameters alone (address_digits says why)
    size_t plan_digits() const {
        size_t bits = 0, n_digits = 0;
        for (size_t v = params.max_addr() - 1; v; v >>= 1) bits++;
        while (bits) {
            const size_t before = bits;
            for (uint32_t i = 0; i < params.p.n_decomp && bits; i++) { bits -= std::min<size_t>(bits, params.p.decomp_n[i]); n_digits++; }
            if (bits == before) throw Error(FHERAM_ERR_INVALID_ARG, "a decomposition without bits");
        }
        return n_digits;
    }
    // the std-form digits of an address of this bank, one vector per digit (fheram_bank_address_download)
    std::vector<std::vector<int64_t>> address_digits(Address& a) {
        // The digit count: the ABI has no bank form of fheram_n_digits, so it is get_base_2d's (base.rs:84-108) on the parameters alone — every
        // coordinate takes the decomposition's widths in turn until the address bits run out.  A count the library disagrees with cannot pass
        // unnoticed: fheram_bank_address_download fills n_digits of its own, and host_check.cpp compares the result's size.
        const size_t n_digits = plan_digits();
        const size_t ggsw = fheram_ggsw_len(nullptr);   // (the layout's length: the library's own figure, which needs no context)
        fheram_addr* h = nullptr;
        for (auto& kv : addr_) if (kv.first == &a) h = kv.second;
        if (!h) h = dev(a);
        std::vector<int64_t> flat(n_digits * ggsw);
        chk(fheram_bank_address_download(bank_, h, flat.data()));
        std::vector<std::vector<int64_t>> out;
        for (size_t d = 0; d < n_digits; d++) out.emplace_back(flat.begin() + d * ggsw, flat.begin() + (d + 1) * ggsw);
        return out;
    }
    static fheram_select_src src_zero() { return {FHERAM_SRC_ZERO, 0}; }
    static fheram_select_src src_host(int slot) { return {FHERAM_SRC_HOST, slot}; }           // slot of host_words
    static fheram_select_src src_member(int member) { return {FHERAM_SRC_MEMBER_RESULT, member}; }
    static fheram_select_src src_list(int entry) { return {FHERAM_SRC_LIST_RESULT, entry}; }
    static fheram_select_src src_select(int output) { return {FHERAM_SRC_SELECT_RESULT, output}; }
    // sels.size() selects as ONE operation (fheram_bank_select): *sels[k] picks one of candidates[k]; result k is the picked word.  The keys are
    // those the bank has loaded (any earlier operation's).  download = false: no host wait, an empty result (select_result later).
    std::vector<std::vector<Glwe>> select(const std::vector<const Selector*>& sels, const std::vector<std::vector<fheram_select_src>>& candidates,
                                          const std::vector<std::vector<Glwe>>& host_words = {}, bool download = true) {
        if (sels.empty() || candidates.size() != sels.size()) throw Error(FHERAM_ERR_INVALID_ARG, "select takes at least one selector and one candidate list per selector");
        std::vector<const fheram_selector*> sh;
        std::vector<int> n_cand;
        std::vector<fheram_select_src> flat_src;
        for (const Selector* x : sels) { if (!x) throw Error(FHERAM_ERR_INVALID_ARG, "null selector"); sh.push_back(x->h_); }
        for (auto& c : candidates) { n_cand.push_back((int)c.size()); flat_src.insert(flat_src.end(), c.begin(), c.end()); }
        std::vector<int64_t> flat;
        for (auto& word : host_words) {
            if (word.size() != params.word_size()) throw Error(FHERAM_ERR_INVALID_ARG, "a host candidate has word_size GLWEs");
            for (auto& g : word) flat.insert(flat.end(), g.begin(), g.end());
        }
        for (auto& x : flat_src)
            if (x.kind == FHERAM_SRC_HOST && (x.index < 0 || (size_t)x.index >= host_words.size())) throw Error(FHERAM_ERR_INVALID_ARG, "a host candidate names a slot outside host_words");
        std::vector<int64_t> out(download ? sh.size() * params.word_size() * glwe_len() : 0);
        chk(fheram_bank_select(bank_, sh.data(), n_cand.data(), (int)sh.size(), flat_src.data(), flat.empty() ? nullptr : flat.data(), download ? out.data() : nullptr));
        return download ? split(out, sh.size()) : std::vector<std::vector<Glwe>>();
    }
    // GLWE `lane` of the word a source names (fheram_select_lane)
    static fheram_select_lane lane_of(fheram_select_src src, int lane) { return {src.kind, src.index, src.kind == FHERAM_SRC_ZERO ? 0 : lane, 0}; }
    // select with lane-mapped candidates (fheram_bank_select_lanes): candidates[k][j] is the word_size lanes candidate j of select k is assembled from
    std::vector<std::vector<Glwe>> select_lanes(const std::vector<const Selector*>& sels, const std::vector<std::vector<std::vector<fheram_select_lane>>>& candidates,
                                                const std::vector<std::vector<Glwe>>& host_words = {}, bool download = true) {
        if (sels.empty() || candidates.size() != sels.size()) throw Error(FHERAM_ERR_INVALID_ARG, "select_lanes takes at least one selector and one candidate list per selector");
        std::vector<const fheram_selector*> sh;
        std::vector<int> n_cand;
        std::vector<fheram_select_lane> flat_lanes;
        for (const Selector* x : sels) { if (!x) throw Error(FHERAM_ERR_INVALID_ARG, "null selector"); sh.push_back(x->h_); }
        for (auto& c : candidates) {
            n_cand.push_back((int)c.size());
            for (auto& word : c) {
                if (word.size() != params.word_size()) throw Error(FHERAM_ERR_INVALID_ARG, "a candidate has word_size lanes");
                flat_lanes.insert(flat_lanes.end(), word.begin(), word.end());
            }
        }
        std::vector<int64_t> flat;
        for (auto& word : host_words) {
            if (word.size() != params.word_size()) throw Error(FHERAM_ERR_INVALID_ARG, "a host candidate has word_size GLWEs");
            for (auto& g : word) flat.insert(flat.end(), g.begin(), g.end());
        }
        for (auto& x : flat_lanes)
            if (x.kind == FHERAM_SRC_HOST && (x.index < 0 || (size_t)x.index >= host_words.size())) throw Error(FHERAM_ERR_INVALID_ARG, "a host lane names a slot outside host_words");
        std::vector<int64_t> out(download ? sh.size() * params.word_size() * glwe_len() : 0);
        chk(fheram_bank_select_lanes(bank_, sh.data(), n_cand.data(), (int)sh.size(), flat_lanes.data(), flat.empty() ? nullptr : flat.data(), download ? out.data() : nullptr));
        return download ? split(out, sh.size()) : std::vector<std::vector<Glwe>>();
    }
    // outputs [first, first + n) of the last select (fheram_bank_select_result)
    std::vector<std::vector<Glwe>> select_result(int first, int n) {
        if (n < 1) throw Error(FHERAM_ERR_INVALID_ARG, "empty slice of the last select");
        std::vector<int64_t> out((size_t)n * params.word_size() * glwe_len());
        chk(fheram_bank_select_result(bank_, first, n, out.data()));
        return split(out, (size_t)n);
    }
    // write_list whose words are outputs of the last select (fheram_bank_write_list_selected): output picks[k] to member members[k] at
    // *addresses[k]; the words never leave the device
    void write_selected(const std::vector<int>& members, const std::vector<int>& picks, std::vector<Address*>& addresses, const EvaluationKeysPrepared& keys) {
        if (members.empty() || addresses.size() != members.size() || picks.size() != members.size())
            throw Error(FHERAM_ERR_INVALID_ARG, "write_selected takes at least one member, as many addresses and one pick per member");
        use(keys);
        std::vector<const fheram_addr*> h = handles(addresses);
        chk(fheram_bank_write_list_selected(bank_, members.data(), h.data(), (int)h.size(), picks.data()));
    }
    // ---- a register file (include/fheram.h): a one-row RAM of 2^bits words beside the members, read and written by the bank's selectors
    static fheram_select_src src_regs(int output) { return {FHERAM_SRC_REGS_RESULT, output}; }   // output of the bank's last RegFile::read
    static fheram_select_src src_regs_old() { return {FHERAM_SRC_REGS_OLD, 0}; }                 // the bank's last RegFile::read_prepare_write result
    class RegFile {
    public:
        struct Wide {};   // RegFile(bank, bits, Wide{}): up to FHERAM_TABLE_BITS_MAX bits, addressed by wide selectors (Bank::scratch)
        RegFile(Bank& bank, int bits) : bank_(bank) { bank.chk(fheram_bank_regs_create(bank.bank_, bits, &h_)); }
        RegFile(Bank& bank, int bits, Wide) : bank_(bank) { bank.chk(fheram_bank_regs_create_wide(bank.bank_, bits, &h_)); }
        ~RegFile() { if (h_) fheram_regs_destroy(h_); }
        RegFile(const RegFile&) = delete;
        int bits() const { return fheram_regs_bits(h_); }
        bool state() const { return fheram_bank_regs_state(bank_.bank_, h_) != 0; }
        // row: [word_size][GLWE], Ram::encrypt_sk's output for the one-row RAM of max_addr = 2^bits
        void load(const std::vector<int64_t>& row) {
            if (row.size() != bank_.params.word_size() * bank_.glwe_len()) throw Error(FHERAM_ERR_INVALID_ARG, "invalid data: expected word_size x 1 GLWE rows (ram.rs:144-155)");
            bank_.chk(fheram_bank_regs_upload(bank_.bank_, h_, row.data()));
        }
        std::vector<int64_t> store() {
            std::vector<int64_t> row(bank_.params.word_size() * bank_.glwe_len());
            bank_.chk(fheram_bank_regs_download(bank_.bank_, h_, row.data()));
            return row;
        }
        // row <- the pack of Bank::select over `sources`, word j at coefficient j
        void pack(const std::vector<fheram_select_src>& sources, const std::vector<std::vector<Glwe>>& host_words = {}) {
            const std::vector<int64_t> flat = bank_.flat_words(sources, host_words);
            bank_.chk(fheram_bank_regs_pack(bank_.bank_, h_, (int)sources.size(), sources.data(), flat.empty() ? nullptr : flat.data()));
        }
        // sels.size() reads as ONE operation; download = false: no host wait, an empty result (result later)
        std::vector<std::vector<Glwe>> read(const std::vector<const Selector*>& sels, bool download = true) {
            std::vector<const fheram_selector*> sh;
            for (const Selector* x : sels) { if (!x) throw Error(FHERAM_ERR_INVALID_ARG, "null selector"); sh.push_back(x->h_); }
            std::vector<int64_t> out(download ? sh.size() * bank_.params.word_size() * bank_.glwe_len() : 0);
            bank_.chk(fheram_bank_regs_read(bank_.bank_, h_, sh.data(), (int)sh.size(), download ? out.data() : nullptr));
            return download ? bank_.split(out, sh.size()) : std::vector<std::vector<Glwe>>();
        }
        std::vector<std::vector<Glwe>> result(int first, int n) {
            if (n < 1) throw Error(FHERAM_ERR_INVALID_ARG, "empty slice of the last register read");
            std::vector<int64_t> out((size_t)n * bank_.params.word_size() * bank_.glwe_len());
            bank_.chk(fheram_bank_regs_result(bank_.bank_, first, n, out.data()));
            return bank_.split(out, (size_t)n);
        }
        // the two halves of a register write: the OLD word; then the word `src` names, written at the prepared index
        std::vector<Glwe> read_prepare_write(const Selector& sel, bool download = true) {
            std::vector<int64_t> out(download ? bank_.params.word_size() * bank_.glwe_len() : 0);
            bank_.chk(fheram_bank_regs_read_prepare_write(bank_.bank_, h_, sel.h_, download ? out.data() : nullptr));
            return download ? bank_.split(out, 1)[0] : std::vector<Glwe>();
        }
        std::vector<Glwe> old_result() {
            std::vector<int64_t> out(bank_.params.word_size() * bank_.glwe_len());
            bank_.chk(fheram_bank_regs_old_result(bank_.bank_, out.data()));
            return bank_.split(out, 1)[0];
        }
        void write(const Selector& sel, fheram_select_src src, const std::vector<std::vector<Glwe>>& host_words = {}) {
            const std::vector<int64_t> flat = bank_.flat_words({src}, host_words);
            bank_.chk(fheram_bank_regs_write(bank_.bank_, h_, sel.h_, src, flat.empty() ? nullptr : flat.data()));
        }
        // Ram::encrypt_sk of the one-row RAM of max_addr = 2^bits, straight into the row: data = 2^bits * word_size bytes
        void encrypt_sk(const std::vector<uint8_t>& data, const Secret& sk, Source& source_xa, Source& source_xe) {
            std::vector<int64_t> mask, noise;
            bank_.rows_draws(1, source_xa, source_xe, mask, noise);
            bank_.chk(fheram_bank_regs_encrypt_sk(bank_.bank_, h_, sk.h_, data.data(), data.size(), mask.data(), noise.data()));
        }
        // every word, decrypted and decoded on the device: [2^bits][word_size]; worst (optional): the worst log2 noise against the decoded values
        std::vector<int32_t> decrypt(const Secret& sk, double* worst = nullptr) {
            std::vector<int32_t> values(((size_t)1 << bits()) * bank_.params.word_size());
            bank_.chk(fheram_bank_regs_decrypt(bank_.bank_, h_, sk.h_, values.data(), worst));
            return values;
        }
        // indices.size() reads at PUBLIC word indices as ONE operation (fheram_bank_regs_peek); the outputs are the bank's last peek
        // (Bank::peek_result, src_peek); download = false: no host wait, an empty result
        std::vector<std::vector<Glwe>> peek(const std::vector<uint32_t>& indices, bool download = true) {
            if (indices.empty()) throw Error(FHERAM_ERR_INVALID_ARG, "peek takes at least one index");
            std::vector<int64_t> out(download ? indices.size() * bank_.params.word_size() * bank_.glwe_len() : 0);
            bank_.chk(fheram_bank_regs_peek(bank_.bank_, h_, indices.data(), (int)indices.size(), download ? out.data() : nullptr));
            return download ? bank_.split(out, indices.size()) : std::vector<std::vector<Glwe>>();
        }
        // indices.size() writes at distinct PUBLIC word indices as ONE operation (fheram_bank_regs_poke): entry k writes the word srcs[k]
        // names; the old words are the bank's last peek afterwards.  Never waits for the device.
        void poke(const std::vector<uint32_t>& indices, const std::vector<fheram_select_src>& srcs, const std::vector<std::vector<Glwe>>& host_words = {}) {
            if (indices.empty() || srcs.size() != indices.size()) throw Error(FHERAM_ERR_INVALID_ARG, "poke takes at least one index and one source per index");
            const std::vector<int64_t> flat = bank_.flat_words(srcs, host_words);
            bank_.chk(fheram_bank_regs_poke(bank_.bank_, h_, indices.data(), (int)indices.size(), srcs.data(), flat.empty() ? nullptr : flat.data()));
        }
    private:
        friend class Bank;
        Bank& bank_;
        fheram_regs* h_ = nullptr;
    };
    // a WIDE register file of 2^bits words, bits <= FHERAM_TABLE_BITS_MAX (fheram_bank_regs_create_wide): a writable one-row memory of up to
    // 4096 words; above FHERAM_SELECT_BITS_MAX bits its addresses are wide selectors (Selector::Wide)
    RegFile scratch(int bits) { return RegFile(*this, bits, RegFile::Wide{}); }
    // ---- a table (include/fheram.h): a READ-ONLY one-row RAM of 2^bits words, bits <= FHERAM_TABLE_BITS_MAX, beside the members and the
    // register files — an instruction ROM or a lookup table — read at wide selectors (Selector::Wide)
    static fheram_select_src src_table(int output) { return {FHERAM_SRC_TABLE_RESULT, output}; }   // output of the bank's last table_read
    class Table {
    public:
        Table(Bank& bank, int bits) : bank_(bank) { bank.chk(fheram_bank_table_create(bank.bank_, bits, &h_)); }
        ~Table() { if (h_) fheram_table_destroy(h_); }
        Table(const Table&) = delete;
        int bits() const { return fheram_table_bits(h_); }
        // row: [word_size][GLWE], Ram::encrypt_sk's output for the one-row RAM of max_addr = 2^bits
        void load(const std::vector<int64_t>& row) {
            if (row.size() != bank_.params.word_size() * bank_.glwe_len()) throw Error(FHERAM_ERR_INVALID_ARG, "invalid data: expected word_size x 1 GLWE rows (ram.rs:144-155)");
            bank_.chk(fheram_bank_table_upload(bank_.bank_, h_, row.data()));
        }
        // public bytes (2^bits * word_size, Ram::encrypt_sk's layout) as the trivial ciphertext: no host encryption, no keys
        void load_plain(const std::vector<uint8_t>& data) { bank_.chk(fheram_bank_table_load_plain(bank_.bank_, h_, data.data(), data.size())); }
        std::vector<int64_t> download() {
            std::vector<int64_t> row(bank_.params.word_size() * bank_.glwe_len());
            bank_.chk(fheram_bank_table_download(bank_.bank_, h_, row.data()));
            return row;
        }
        // Ram::encrypt_sk of the one-row RAM of max_addr = 2^bits, straight into the row: data = 2^bits * word_size bytes
        void encrypt_sk(const std::vector<uint8_t>& data, const Secret& sk, Source& source_xa, Source& source_xe) {
            std::vector<int64_t> mask, noise;
            bank_.rows_draws(1, source_xa, source_xe, mask, noise);
            bank_.chk(fheram_bank_table_encrypt_sk(bank_.bank_, h_, sk.h_, data.data(), data.size(), mask.data(), noise.data()));
        }
        // every word, decrypted and decoded on the device: [2^bits][word_size]; worst (optional): the worst log2 noise against the decoded values
        std::vector<int32_t> decrypt(const Secret& sk, double* worst = nullptr) {
            std::vector<int32_t> values(((size_t)1 << bits()) * bank_.params.word_size());
            bank_.chk(fheram_bank_table_decrypt(bank_.bank_, h_, sk.h_, values.data(), worst));
            return values;
        }
    private:
        friend class Bank;
        Bank& bank_;
        fheram_table* h_ = nullptr;
    };
    // sels.size() reads as ONE operation (fheram_bank_table_read): entry k reads *tables[k] at *sels[k]; download = false: no host wait, an
    // empty result (table_result later)
    std::vector<std::vector<Glwe>> table_read(const std::vector<const Table*>& tables, const std::vector<const Selector*>& sels, bool download = true) {
        if (sels.empty() || tables.size() != sels.size()) throw Error(FHERAM_ERR_INVALID_ARG, "table_read takes at least one selector and one table per selector");
        std::vector<const fheram_table*> th;
        std::vector<const fheram_selector*> sh;
        for (const Table* t : tables) { if (!t) throw Error(FHERAM_ERR_INVALID_ARG, "null table"); th.push_back(t->h_); }
        for (const Selector* x : sels) { if (!x) throw Error(FHERAM_ERR_INVALID_ARG, "null selector"); sh.push_back(x->h_); }
        std::vector<int64_t> out(download ? sh.size() * params.word_size() * glwe_len() : 0);
        chk(fheram_bank_table_read(bank_, th.data(), sh.data(), (int)sh.size(), download ? out.data() : nullptr));
        return download ? split(out, sh.size()) : std::vector<std::vector<Glwe>>();
    }
    // outputs [first, first + n) of the last table read (fheram_bank_table_result)
    std::vector<std::vector<Glwe>> table_result(int first, int n) {
        if (n < 1) throw Error(FHERAM_ERR_INVALID_ARG, "empty slice of the last table read");
        std::vector<int64_t> out((size_t)n * params.word_size() * glwe_len());
        chk(fheram_bank_table_result(bank_, first, n, out.data()));
        return split(out, (size_t)n);
    }
    // ---- the public side (include/fheram.h): plain image loads, peek and poke at PUBLIC word addresses
    static fheram_select_src src_peek(int output) { return {FHERAM_SRC_PEEK_RESULT, output}; }   // output of the bank's last peek / old word of its last poke
    // public bytes (whole words, Ram::encrypt_sk's layout) into the rows of one member from first_row on, as the trivial ciphertexts: no host
    // encryption, no keys.  data covers whole rows, or ends where the member does; first_row = 0 with max_addr words loads the whole member.
    void load_plain(int member, const std::vector<uint8_t>& data, size_t first_row = 0) {
        const size_t ws = params.word_size(), n = params.n(), words = data.size() / ws;
        if (data.empty() || data.size() % ws) throw Error(FHERAM_ERR_INVALID_ARG, "invalid data: not a positive number of words");
        chk(fheram_bank_ram_load_plain(bank_, member, first_row, (words + n - 1) / n, data.data(), data.size()));
    }
    void load_plain(RegFile& regs, const std::vector<uint8_t>& data) { chk(fheram_bank_regs_load_plain(bank_, regs.h_, data.data(), data.size())); }
    // members.size() reads at public addresses as ONE operation (fheram_bank_peek); download = false: no host wait, an empty result (peek_result later)
    std::vector<std::vector<Glwe>> peek(const std::vector<int>& members, const std::vector<uint64_t>& addresses, bool download = true) {
        if (members.empty() || addresses.size() != members.size()) throw Error(FHERAM_ERR_INVALID_ARG, "peek takes at least one member and one address per member");
        std::vector<int64_t> out(download ? members.size() * params.word_size() * glwe_len() : 0);
        chk(fheram_bank_peek(bank_, members.data(), addresses.data(), (int)members.size(), download ? out.data() : nullptr));
        return download ? split(out, members.size()) : std::vector<std::vector<Glwe>>();
    }
    std::vector<std::vector<Glwe>> peek_result(int first, int n) {
        if (n < 1) throw Error(FHERAM_ERR_INVALID_ARG, "empty slice of the last peek");
        std::vector<int64_t> out((size_t)n * params.word_size() * glwe_len());
        chk(fheram_bank_peek_result(bank_, first, n, out.data()));
        return split(out, (size_t)n);
    }
    // members.size() writes at public addresses as ONE operation (fheram_bank_poke): entry k writes the word srcs[k] names (src_host(i): slot i
    // of host_words); the old words are the last peek afterwards.  Never waits for the device.
    void poke(const std::vector<int>& members, const std::vector<uint64_t>& addresses, const std::vector<fheram_select_src>& srcs,
              const std::vector<std::vector<Glwe>>& host_words = {}) {
        if (members.empty() || addresses.size() != members.size() || srcs.size() != members.size())
            throw Error(FHERAM_ERR_INVALID_ARG, "poke takes at least one member, and one address and one source per member");
        const std::vector<int64_t> flat = flat_words(srcs, host_words);
        chk(fheram_bank_poke(bank_, members.data(), addresses.data(), (int)members.size(), srcs.data(), flat.empty() ? nullptr : flat.data()));
    }
    // ---- mixed reads (include/fheram.h): a read list, a table read and a register read as ONE operation with one top.  A group
    // may be empty (regs: nullptr and no selectors) but not all three; at most FHERAM_MIX_MAX entries in all.  Entry k of a group equals
    // output k of read_list / table_read / RegFile::read, and list_result / table_result / RegFile::result read the groups' outputs afterwards.
    struct MixResult { std::vector<std::vector<Glwe>> list, table, regs; };   // (download = false: all empty)
    MixResult read_mix(const std::vector<int>& members, std::vector<Address*>& addresses, const std::vector<const Table*>& tables,
                       const std::vector<const Selector*>& table_sels, const RegFile* regs, const std::vector<const Selector*>& reg_sels,
                       const EvaluationKeysPrepared& keys, bool download = true) {
        if (addresses.size() != members.size() || table_sels.size() != tables.size())
            throw Error(FHERAM_ERR_INVALID_ARG, "read_mix takes as many addresses as members and as many selectors as tables");
        const size_t nl = members.size(), nt = tables.size(), nr = reg_sels.size();
        if (nl + nt + nr < 1) throw Error(FHERAM_ERR_INVALID_ARG, "read_mix takes at least one read: all three groups are empty");
        if (nl + nt + nr > FHERAM_MIX_MAX) throw Error(FHERAM_ERR_INVALID_ARG, "read_mix takes at most FHERAM_MIX_MAX entries in all");
        if (nr && !regs) throw Error(FHERAM_ERR_INVALID_ARG, "the regs group of read_mix takes a register file");
        use(keys);
        std::vector<const fheram_addr*> ah = handles(addresses);
        std::vector<const fheram_table*> th;
        std::vector<const fheram_selector*> tsh, rsh;
        for (const Table* t : tables) { if (!t) throw Error(FHERAM_ERR_INVALID_ARG, "null table"); th.push_back(t->h_); }
        for (const Selector* x : table_sels) { if (!x) throw Error(FHERAM_ERR_INVALID_ARG, "null selector"); tsh.push_back(x->h_); }
        for (const Selector* x : reg_sels) { if (!x) throw Error(FHERAM_ERR_INVALID_ARG, "null selector"); rsh.push_back(x->h_); }
        const fheram_mix_reads reads{members.data(), ah.data(), (int)nl, th.data(), tsh.data(), (int)nt, nr ? regs->h_ : nullptr, rsh.data(), (int)nr};
        const size_t one = params.word_size() * glwe_len();
        std::vector<int64_t> lo(download ? nl * one : 0), to(download ? nt * one : 0), ro(download ? nr * one : 0);
        chk(fheram_bank_read_mix(bank_, &reads, lo.empty() ? nullptr : lo.data(), to.empty() ? nullptr : to.data(), ro.empty() ? nullptr : ro.data()));
        MixResult res;
        if (download) {
            if (nl) res.list = split(lo, nl);
            if (nt) res.table = split(to, nt);
            if (nr) res.regs = split(ro, nr);
        }
        return res;
    }
    // ---- the reads of a step and the first halves of its writes under ONE top (include/fheram.h).  The read groups are
    // read_mix's and may all be empty; prep_members / prep_addresses: distinct members, as read_prepare_write_list; prep_regs / prep_sel: as
    // RegFile::read_prepare_write (nullptr, nullptr: none).  At least one preparation, at most FHERAM_MIX_MAX entries in all (the register
    // file counts 1).  Equals read_mix, read_prepare_write_list, RegFile::read_prepare_write in that order.
    struct PrepareMixResult { MixResult reads; std::vector<std::vector<Glwe>> prep_list; std::vector<Glwe> prep_regs; };   // the OLD words
    PrepareMixResult read_prepare_write_mix(const std::vector<int>& members, std::vector<Address*>& addresses, const std::vector<const Table*>& tables,
                                            const std::vector<const Selector*>& table_sels, const RegFile* regs, const std::vector<const Selector*>& reg_sels,
                                            const std::vector<int>& prep_members, std::vector<Address*>& prep_addresses, RegFile* prep_regs,
                                            const Selector* prep_sel, const EvaluationKeysPrepared& keys, bool download = true) {
        if (addresses.size() != members.size() || table_sels.size() != tables.size() || prep_addresses.size() != prep_members.size())
            throw Error(FHERAM_ERR_INVALID_ARG, "read_prepare_write_mix takes as many addresses as members and as many selectors as tables");
        const size_t nl = members.size(), nt = tables.size(), nr = reg_sels.size(), np = prep_members.size(), npr = prep_regs ? 1 : 0;
        if (np + npr < 1) throw Error(FHERAM_ERR_INVALID_ARG, "read_prepare_write_mix takes at least one preparation (without one it is read_mix)");
        if (nl + nt + nr + np + npr > FHERAM_MIX_MAX) throw Error(FHERAM_ERR_INVALID_ARG, "read_prepare_write_mix takes at most FHERAM_MIX_MAX entries in all");
        if (nr && !regs) throw Error(FHERAM_ERR_INVALID_ARG, "the regs group of read_prepare_write_mix takes a register file");
        if ((prep_regs != nullptr) != (prep_sel != nullptr)) throw Error(FHERAM_ERR_INVALID_ARG, "a prepared register file takes one selector");
        use(keys);
        std::vector<const fheram_addr*> ah = handles(addresses), pah = handles(prep_addresses);
        std::vector<const fheram_table*> th;
        std::vector<const fheram_selector*> tsh, rsh;
        for (const Table* t : tables) { if (!t) throw Error(FHERAM_ERR_INVALID_ARG, "null table"); th.push_back(t->h_); }
        for (const Selector* x : table_sels) { if (!x) throw Error(FHERAM_ERR_INVALID_ARG, "null selector"); tsh.push_back(x->h_); }
        for (const Selector* x : reg_sels) { if (!x) throw Error(FHERAM_ERR_INVALID_ARG, "null selector"); rsh.push_back(x->h_); }
        const fheram_mix_reads reads{members.data(), ah.data(), (int)nl, th.data(), tsh.data(), (int)nt, nr ? regs->h_ : nullptr, rsh.data(), (int)nr};
        const fheram_mix_prepares prepares{prep_members.data(), pah.data(), (int)np, npr ? prep_regs->h_ : nullptr, npr ? prep_sel->h_ : nullptr};
        const size_t one = params.word_size() * glwe_len();
        std::vector<int64_t> lo(download ? nl * one : 0), to(download ? nt * one : 0), ro(download ? nr * one : 0), po(download ? np * one : 0), pr(download ? npr * one : 0);
        auto ptr = [](std::vector<int64_t>& v) { return v.empty() ? nullptr : v.data(); };
        chk(fheram_bank_read_prepare_write_mix(bank_, &reads, &prepares, ptr(lo), ptr(to), ptr(ro), ptr(po), ptr(pr)));
        PrepareMixResult res;
        if (download) {
            if (nl) res.reads.list = split(lo, nl);
            if (nt) res.reads.table = split(to, nt);
            if (nr) res.reads.regs = split(ro, nr);
            if (np) res.prep_list = split(po, np);
            if (npr) res.prep_regs = split(pr, 1)[0];
        }
        return res;
    }
    // ---- the setup side, continued: keys, members, addresses, words; decryption of what the bank leaves on the device
    // EvaluationKeys::encrypt_sk + prepare on the bank (fheram_bank_keys_encrypt_sk); `keys` is marked as the set in use (its std forms stay empty)
    void encrypt_keys(EvaluationKeysPrepared& keys, const Secret& sk, Source& source_xa, Source& source_xe) {
        const size_t n = params.n(), b = params.basek();
        const size_t s4 = (params.p.k_evk_trace + b - 1) / b, s5 = (params.p.k_evk_ggsw_inv + b - 1) / b;
        const size_t dnum_ct = (params.k_glwe_ct() + b - 1) / b, dnum_ggsw = (params.p.k_ggsw_addr + b - 1) / b;   // parameters.rs:273-279
        const size_t n4 = params.p.log_n * dnum_ct, n5 = 2 * dnum_ggsw;
        std::vector<int64_t> mask((n4 * s4 + n5 * s5) * n), noise((n4 + n5) * n);
        source_xa.uniform_limbs(mask.data(), n4 * s4 * n);
        source_xa.uniform_limbs(mask.data() + n4 * s4 * n, n5 * s5 * n);
        source_xe.gaussian(noise.data(), n4 * n, noise_scale(params.p.k_evk_trace, params.basek()));
        source_xe.gaussian(noise.data() + n4 * n, n5 * n, noise_scale(params.p.k_evk_ggsw_inv, params.basek()));
        chk(fheram_bank_keys_encrypt_sk(bank_, sk.h_, mask.data(), noise.data(), nullptr));
        keys_ = &keys;
    }
    // Ram::encrypt_sk of one member, straight into its rows (fheram_bank_ram_encrypt_sk): data = max_addr * word_size bytes
    void encrypt_sk(int member, const std::vector<uint8_t>& data, const Secret& sk, Source& source_xa, Source& source_xe) {
        std::vector<int64_t> mask, noise;
        rows_draws((params.max_addr() + params.n() - 1) / params.n(), source_xa, source_xe, mask, noise);
        chk(fheram_bank_ram_encrypt_sk(bank_, member, sk.h_, data.data(), data.size(), mask.data(), noise.data()));
    }
    // Address::encrypt_sk on the bank (fheram_bank_address_encrypt_sk): *a becomes an ordinary address of this bank
    void encrypt_address(Address& a, uint32_t value, const Secret& sk, Source& source_xa, Source& source_xe) {
        const size_t n = params.n(), b = params.basek(), size = (params.p.k_ggsw_addr + b - 1) / b;
        const size_t glwes = (size_t)plan_digits() * ((params.k_glwe_ct() + b - 1) / b) * 2;   // dnum_ct rows x 2
        std::vector<int64_t> mask(glwes * size * n), noise(glwes * n);
        source_xa.uniform_limbs(mask.data(), mask.size());
        source_xe.gaussian(noise.data(), noise.size(), noise_scale(params.p.k_ggsw_addr, (uint32_t)b));
        fheram_addr* h = nullptr;
        chk(fheram_bank_address_encrypt_sk(bank_, sk.h_, value, mask.data(), noise.data(), &h));
        for (auto& kv : addr_) if (kv.first == &a) { fheram_address_destroy(kv.second); kv.second = h; h = nullptr; }
        if (h) addr_.emplace_back(&a, h);
        a.digits.clear();
    }
    // encrypt_glwe of the example (examples/fhe-ram.rs:179-210) on the bank's secret: one GLWE per byte, value on coefficient 0 at precision k_pt
    std::vector<Glwe> encrypt_word(const std::vector<uint8_t>& bytes, const Secret& sk, Source& source_xa, Source& source_xe) {
        const size_t n = params.n(), b = params.basek(), size = (params.k_glwe_ct() + b - 1) / b, k_pt = params.p.k_glwe_pt, size_pt = (k_pt + b - 1) / b;
        std::vector<int64_t> pt(bytes.size() * size_pt * n, 0), mask(bytes.size() * size * n), noise(bytes.size() * n), out(bytes.size() * size * 2 * n);
        for (size_t i = 0; i < bytes.size(); i++) {   // encode_coeff_i64(value, k_pt, 0)
            int64_t x = (int64_t)((uint64_t)bytes[i] << (size_pt * b - k_pt));
            for (size_t j = size_pt; j-- > 0;) {
                const int64_t half = (int64_t)1 << (b - 1), d = ((x + half) & (((int64_t)1 << b) - 1)) - half;
                pt[(i * size_pt + j) * n] = d;
                x = (x - d) >> b;
            }
        }
        source_xa.uniform_limbs(mask.data(), mask.size());
        source_xe.gaussian(noise.data(), noise.size(), noise_scale(params.k_glwe_ct(), (uint32_t)b));
        chk(fheram_bank_glwe_encrypt_sk(bank_, sk.h_, (int)bytes.size(), (int)size, (int)params.k_glwe_ct(), pt.data(), (int)size_pt, 0, mask.data(), noise.data(), out.data()));
        std::vector<Glwe> res;
        for (size_t i = 0; i < bytes.size(); i++) res.emplace_back(out.begin() + i * glwe_len(), out.begin() + (i + 1) * glwe_len());
        return res;
    }
    // GLWE::decrypt of downloaded ciphertexts on the bank's secret (fheram_bank_glwe_decrypt): normalised plaintext limbs [n][size][N]
    std::vector<int64_t> decrypt(const std::vector<Glwe>& cts, const Secret& sk) {
        std::vector<int64_t> flat, pt(cts.size() * glwe_len() / 2);
        for (auto& g : cts) flat.insert(flat.end(), g.begin(), g.end());
        chk(fheram_bank_glwe_decrypt(bank_, sk.h_, (int)cts.size(), (int)(glwe_len() / (2 * params.n())), flat.data(), pt.data()));
        return pt;
    }
    // coefficient 0 of the words `srcs` name (src_member / src_list / src_select / src_regs / src_regs_old / src_table), decrypted and decoded on
    // the device (fheram_bank_source_decrypt): values [n][word_size]; wants: the expected values or empty; log2_noise (optional): [n][word_size]
    std::vector<int64_t> decrypt_sources(const Secret& sk, const std::vector<fheram_select_src>& srcs, const std::vector<int64_t>& wants = {}, std::vector<double>* log2_noise = nullptr) {
        const size_t cnt = srcs.size() * params.word_size();
        if (srcs.empty() || (!wants.empty() && wants.size() != cnt)) throw Error(FHERAM_ERR_INVALID_ARG, "decrypt_sources takes at least one source and no or n x word_size wants");
        std::vector<int64_t> values(cnt);
        if (log2_noise) log2_noise->assign(cnt, 0.0);
        chk(fheram_bank_source_decrypt(bank_, sk.h_, srcs.data(), (int)srcs.size(), wants.empty() ? nullptr : wants.data(), values.data(), log2_noise ? log2_noise->data() : nullptr));
        return values;
    }
    // every word of one member, decrypted and decoded on the device (fheram_bank_ram_decrypt): [max_addr][word_size]
    std::vector<int32_t> decrypt(int member, const Secret& sk, double* worst = nullptr) {
        std::vector<int32_t> values(params.max_addr() * params.word_size());
        chk(fheram_bank_ram_decrypt(bank_, member, sk.h_, values.data(), worst));
        return values;
    }
    void sync() { chk(fheram_bank_sync(bank_)); }
    double roundoff_max() { double m = 0.0; chk(fheram_bank_roundoff_max(bank_, &m)); return m; }
    struct ChainStats { uint64_t launches = 0, redone = 0; };
    ChainStats tail_stats() { ChainStats s; chk(fheram_bank_tail_stats(bank_, &s.launches, &s.redone)); return s; }
    ChainStats mid_stats() { ChainStats s; chk(fheram_bank_mid_stats(bank_, &s.launches, &s.redone)); return s; }

private:
    fheram_bank* bank_ = nullptr;
    // the draws of Ram::encrypt_sk for `rows` rows per word, in the reference's order
    void rows_draws(size_t rows, Source& source_xa, Source& source_xe, std::vector<int64_t>& mask, std::vector<int64_t>& noise) const {
        const size_t n = params.n(), glwes = params.word_size() * rows, size = (params.k_glwe_ct() + params.basek() - 1) / params.basek();
        mask.resize(glwes * size * n); noise.resize(glwes * n);
        source_xa.uniform_limbs(mask.data(), mask.size());
        source_xe.gaussian(noise.data(), noise.size(), noise_scale(params.k_glwe_ct(), params.basek()));
    }
    // host_words back to back, with every HOST slot the sources name inside them
    std::vector<int64_t> flat_words(const std::vector<fheram_select_src>& sources, const std::vector<std::vector<Glwe>>& host_words) const {
        std::vector<int64_t> flat;
        for (auto& word : host_words) {
            if (word.size() != params.word_size()) throw Error(FHERAM_ERR_INVALID_ARG, "a host word has word_size GLWEs");
            for (auto& g : word) flat.insert(flat.end(), g.begin(), g.end());
        }
        for (auto& x : sources)
            if (x.kind == FHERAM_SRC_HOST && (x.index < 0 || (size_t)x.index >= host_words.size())) throw Error(FHERAM_ERR_INVALID_ARG, "a host source names a slot outside host_words");
        return flat;
    }
    const EvaluationKeysPrepared* keys_ = nullptr;
    std::vector<std::pair<const Address*, fheram_addr*>> addr_;   // device copies bound to the bank, by host address object
    void chk(int rc) { if (rc != FHERAM_OK) throw Error(rc, fheram_bank_last_error(bank_)); }
    void use(const EvaluationKeysPrepared& k) {
        if (keys_ == &k) return;
        std::vector<const int64_t*> ptr;
        for (auto& a : k.atk_glwe) ptr.push_back(a.data());
        chk(fheram_bank_keys_load(bank_, k.gal_els.data(), (int)k.gal_els.size(), ptr.data(), k.atk_ggsw_inv.data(), k.atk_ggsw_inv_p,
                                  k.tsk_ggsw_inv.data()));
        keys_ = &k;
    }
    fheram_addr* dev(const Address& a) {
        for (auto& kv : addr_) if (kv.first == &a) return kv.second;
        std::vector<const int64_t*> ptr;
        for (auto& d : a.digits) ptr.push_back(d.data());
        fheram_addr* h = nullptr;
        chk(fheram_bank_address_create(bank_, ptr.data(), (int)ptr.size(), &h));   // layout check of ram.rs:404
        addr_.emplace_back(&a, h);
        return h;
    }
    std::vector<const fheram_addr*> handles(std::vector<Address*>& addresses) {
        if (addresses.empty()) throw Error(FHERAM_ERR_INVALID_ARG, "empty member range");
        std::vector<const fheram_addr*> h;
        for (Address* a : addresses) {
            if (!a) throw Error(FHERAM_ERR_INVALID_ARG, "null address");
            h.push_back(dev(*a));
        }
        return h;
    }
    std::vector<std::vector<Glwe>> read_op(bool prepare_write, std::vector<Address*>& addresses, const EvaluationKeysPrepared& keys, int first) {
        use(keys);
        std::vector<const fheram_addr*> h = handles(addresses);
        std::vector<int64_t> out(h.size() * params.word_size() * glwe_len());
        chk(prepare_write ? fheram_bank_read_prepare_write(bank_, first, (int)h.size(), h.data(), out.data())
                          : fheram_bank_read(bank_, first, (int)h.size(), h.data(), out.data()));
        return split(out, h.size());
    }
    std::vector<std::vector<Glwe>> split(const std::vector<int64_t>& out, size_t n) const {   // [n][word_size][GLWE]
        const size_t g = glwe_len(), one = params.word_size() * g;
        std::vector<std::vector<Glwe>> res(n);
        for (size_t k = 0; k < n; k++)
            for (size_t i = 0; i < params.word_size(); i++)
                res[k].emplace_back(out.begin() + k * one + i * g, out.begin() + k * one + (i + 1) * g);
        return res;
    }
};

}  // namespace fheram
