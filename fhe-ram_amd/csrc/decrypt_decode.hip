// k_decrypt_decode: GLWE::decrypt (examples/fhe-ram.rs:217-222) and decode_coeff_i64 + the example's noise metric (:224-237) of
// ciphertexts that are ALREADY on the device and stay untouched: a bank's results, a member's rows, a register file's or a table's row.
// Modelled on k_encrypt_sk<S, 1> (kernels.hpp), with two differences:
//   - the ciphertext is read through a const pointer and never written (k_encrypt_sk works in place, which would destroy a member's rows);
//   - the S normalised phase digits of each of the thread's E coefficients stay in registers and are decoded there, in exact integers:
//       res   = the integer decode_coeff_i64(k, i) forms from the digits (the k % base2k != 0 case included)
//       value = res / 2^(k - k_pt), rounded half away from zero
//       diff  = res - (want << (k - k_pt)),  want: the caller's for coefficient 0, else the coefficient's own decoded value
//     Per ciphertext: value (int32) of every coefficient asked for, optionally diff of each, and max |diff| over them as ONE int64 — a
//     wave reduction, then a workgroup reduction through LDS (the exchange buffer, behind a barrier: the transforms are over), one store.
// One 512-thread workgroup per ciphertext, the project's transforms and LDS layout, the round-off monitor at the top.  Plain C++ and
// vector loads and stores only; nothing waits for another workgroup.
// A translation unit of its own (decrypt_decode.hpp says why); the argument struct and the two host entry points are declared there.
#undef FK_STAMP   // (the stamp buffer of the diagnostic build belongs to fheram.hip)
#define FK_NO_PLAIN_KERNELS
#include "kernels.hpp"
#include "decrypt_decode.hpp"

namespace fk {

template <int S>
__global__ __launch_bounds__(T, T / 256) void k_decrypt_decode(DecryptDecodeArgs da) {
    static_assert(S == 3, "a bank's words and rows have 3 limbs; decode_coeff_i64 below walks exactly ceil(k / base2k) = 3 digits");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    RoMonitor ro_mon(lds, da.tw);
    double* tw = lds;
    double* data = lds + LDS_TW;
    const int tid = vt((int)threadIdx.x);
    load_twiddles(tw, da.tw, tid);
    const int x = (int)blockIdx.x;
    const int32_t* cp = da.base ? da.base + (long)x * (S * 2 * N) : da.src[x];   // (workgroup uniform)
    OpRegs sh;
    load_ops(sh, da.s_hat, tid);
    double carry[E];
    int dg[S][E];
#pragma unroll
    for (int k = 0; k < E; k++) carry[k] = 0.0;
#pragma unroll
    for (int j = S - 1; j >= 0; j--) {   // normalise(body + mask * s), limb by limb from the least significant one: k_encrypt_sk<S, 1>
        const int32_t* body = cp + glwe_off(j, 0);
        const int32_t* mask = cp + glwe_off(j, 1);
        int mi[E], bi[E];
#pragma unroll
        for (int k = 0; k < E; k++) { mi[k] = mask[tid + T * k]; bi[k] = body[tid + T * k]; }
        double xr[1][E], acc[1][E];
#pragma unroll
        for (int k = 0; k < E; k++) { xr[0][k] = (double)mi[k]; acc[0][k] = 0.0; }
        ntt_fwd<1>(xr, tw, data, tid);
        mac_regs(acc[0], xr[0], sh);
        ntt_inv<1, false>(acc, tw, data, tid);   // follows a forward transform, whose cross-wave reads are fenced
#pragma unroll
        for (int k = 0; k < E; k++) {
            const double v = (double)bi[k] + acc[0][k] + carry[k];
            const double cy = carry_of(v);
            carry[k] = cy;
            dg[j][k] = (int)digit_of(v, cy);
        }
    }
    // decode_coeff_i64(k, i) and the noise metric (examples/fhe-ram.rs:224-237), exact integers
    const int rem = BASE2K - (da.k % BASE2K);
    const int ls = da.k - da.k_pt;                                                        // :228
    const int count = x == (int)gridDim.x - 1 ? da.n_coef_last : da.n_coef;
    unsigned long long worst = 0;
#pragma unroll
    for (int k = 0; k < E; k++) {
        const int i = tid + T * k;
        const long long hi = (long long)dg[0][k] * (1ll << BASE2K) + dg[1][k];
        const long long res = rem != BASE2K ? hi * (1ll << (BASE2K - rem)) + (long long)(dg[2][k] >> rem) : hi * (1ll << BASE2K) + dg[2][k];
        long long mag = res < 0 ? -res : res;
        if (ls > 0) mag = (mag + (1ll << (ls - 1))) >> ls;                                // round half away from zero  :232-233
        const long long val = res < 0 ? -mag : mag;
        const long long want = (da.has_want && i == 0) ? da.want[x] : val;
        const long long diff = res - (long long)((unsigned long long)want << ls);         // :230
        if (i < count) {
            da.values[(long)x * da.n_coef + i] = (int)val;
            if (da.diff) da.diff[(long)x * da.n_coef + i] = diff;
            const unsigned long long a = (unsigned long long)(diff < 0 ? -diff : diff);
            worst = a > worst ? a : worst;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)worst, off, 64);
        worst = o > worst ? o : worst;
    }
    __syncthreads();   // every wave's last transform is over: the exchange buffer is free
    unsigned long long* red = reinterpret_cast<unsigned long long*>(data);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = worst;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0;
#pragma unroll
        for (int w = 0; w < T / 64; w++) m = red[w] > m ? red[w] : m;
        da.max_diff[x] = (long long)m;
    }
}

hipError_t decrypt_decode_register() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_decrypt_decode<3>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
}
void decrypt_decode_launch(int n_ct, hipStream_t stream, const DecryptDecodeArgs& da) {
    hipLaunchKernelGGL((k_decrypt_decode<3>), dim3(n_ct), dim3(T), LDS_BYTES, stream, da);
}

}  // namespace fk
