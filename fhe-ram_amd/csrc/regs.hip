// The two elementwise kernels of a bank's register file (regs.hpp): a one-row RAM of 2^bits words whose row persists on the device.
//   k_regs_fan    out[k * ws + w] = row[w] for the n entries of a fheram_bank_regs_read: the chain launchers take one source ciphertext per
//                 output, so the n reads of the one row start from n copies of it (ONE launch, whatever n is)
//   k_regs_merge  row[w] = glwe_normalize(row[w] - tr[w] + src[w]): write_first_step (ram.rs:544-577) on the rotated row, with the written
//                 word taken through a per-ciphertext pointer in the argument struct (nullptr: the all-zero ciphertext) — no staging copy,
//                 no zero buffer.  The limb arithmetic is k_sub_add_norm<3>'s: the int32 sum, then one carry pass over the 3 limbs from the
//                 least significant one (normalize_coeff).
// Both cover a ciphertext as the elementwise kernels do (REGS_SLICES workgroups of 256 threads).  Plain vector loads and stores only.
// A translation unit of its own, as k_select_pack and k_cmux_chain are (select_pack.hpp, cmux_chain.hpp): compiled apart it leaves the
// device code of every other kernel exactly as it was.
#undef FK_STAMP
#define FK_NO_PLAIN_KERNELS
#define FK_REGS_KERNELS_ONLY
#include "kernels.hpp"
#include "regs.hpp"

namespace fk {

__global__ __launch_bounds__(256) void k_regs_fan(RegsFanArgs fa) {
    constexpr int S = 3;
    const int y = (int)blockIdx.y, w = y % fa.ws;
    const int4* ap = reinterpret_cast<const int4*>(fa.row + (long)w * (S * 2 * N));
    int4* op = reinterpret_cast<int4*>(fa.out + (long)y * (S * 2 * N));
    for (int idx = blockIdx.z * blockDim.x + threadIdx.x; idx < S * 2 * N / 4; idx += blockDim.x * gridDim.z) op[idx] = ap[idx];
}

__global__ __launch_bounds__(256) void k_regs_merge(RegsMergeArgs ma) {
    constexpr int S = 3;
    const int w = (int)blockIdx.y;
    const long ct = (long)w * (S * 2 * N);
    int32_t* rp = ma.row + ct;
    const int32_t* tp = ma.tr + ct;
    const int32_t* sp = ma.src[w];   // (uniform: the table is the launch's)
    for (int idx = blockIdx.z * blockDim.x + threadIdx.x; idx < 2 * N; idx += blockDim.x * gridDim.z) {
        const int col = idx >> LOGN, i = idx & (N - 1);
        double in_l[S], out_l[S];
#pragma unroll
        for (int j = 0; j < S; j++) {
            const long o = glwe_off(j, col) + i;
            in_l[j] = (double)(rp[o] - tp[o] + (sp ? sp[o] : 0));
        }
        normalize_coeff<S, S>(in_l, out_l);
#pragma unroll
        for (int j = 0; j < S; j++) rp[glwe_off(j, col) + i] = (int)out_l[j];
    }
}

void regs_fan_launch(int n_ct, hipStream_t stream, const RegsFanArgs& fa) {
    hipLaunchKernelGGL(k_regs_fan, dim3(1, n_ct, REGS_SLICES), dim3(256), 0, stream, fa);
}
void regs_merge_launch(int ws, hipStream_t stream, const RegsMergeArgs& ma) {
    hipLaunchKernelGGL(k_regs_merge, dim3(1, ws, REGS_SLICES), dim3(256), 0, stream, ma);
}

}  // namespace fk
