// The two elementwise kernels of a bank's tables (table.hpp): read-only one-row RAMs of up to N words whose rows persist on the device.
//   k_table_fan     out[y] = *src[y] for the n * ws chain inputs of a fheram_bank_table_read: entry k may name any table of the bank, so
//                   the source is a per-ciphertext pointer in the argument struct (k_regs_fan has one row for all).  ONE launch, whatever n is.
//   k_table_encode  row[w] = the trivial ciphertext of byte w of every word: mask limbs 0, body limbs encode_value's (setup.hpp; ram.rs:358-368)
//                   for coefficient j < n_words and 0 behind — what fheram_ram_encrypt_sk stages before k_encrypt_sk, which with an all-zero
//                   mask and noise adds nothing and normalises limbs that are normalised already.  Integer arithmetic only.
// Both cover a ciphertext as the elementwise kernels do (TABLE_SLICES workgroups of 256 threads).  Plain vector loads and stores only: no
// LDS, nothing that waits for another workgroup.
// A translation unit of its own, as k_regs_fan and k_select_pack are (regs.hip, select_pack.hip): compiled apart it leaves the device code
// of every other kernel exactly as it was.
#undef FK_STAMP
#define FK_NO_PLAIN_KERNELS
#define FK_TABLE_KERNELS_ONLY
#include "kernels.hpp"
#include "table.hpp"

namespace fk {

__global__ __launch_bounds__(256) void k_table_fan(TableFanArgs fa) {
    constexpr int S = 3;
    const int y = (int)blockIdx.y;
    const int4* ap = reinterpret_cast<const int4*>(fa.src[y]);   // (uniform: the table is the launch's)
    int4* op = reinterpret_cast<int4*>(fa.out + (long)y * (S * 2 * N));
    for (int idx = blockIdx.z * blockDim.x + threadIdx.x; idx < S * 2 * N / 4; idx += blockDim.x * gridDim.z) op[idx] = ap[idx];
}

// limb j of encode_value(v, k_pt, size_pt) (setup.hpp), j < size_pt: v * 2^-k_pt on the torus in balanced base-2^17 digits
__device__ __forceinline__ void table_encode_value(int v, int k_pt, int size_pt, int (&limbs)[3]) {
    long long x = (long long)((unsigned long long)(long long)v << (size_pt * BASE2K - k_pt)), carry = 0;
#pragma unroll
    for (int j = 2; j >= 0; j--) {
        limbs[j] = 0;
        if (j >= size_pt) continue;
        const long long t = (j == size_pt - 1 ? x : 0) + carry;
        const long long d = (long long)((unsigned long long)t << (64 - BASE2K)) >> (64 - BASE2K);
        limbs[j] = (int)d;
        carry = (t - d) >> BASE2K;
    }
}

__global__ __launch_bounds__(256) void k_table_encode(TableEncodeArgs ea) {
    constexpr int S = 3;
    const int w = (int)blockIdx.y;
    int32_t* rp = ea.row + (long)w * (S * 2 * N);
    for (int q = blockIdx.z * blockDim.x + threadIdx.x; q < N / 4; q += blockDim.x * gridDim.z) {   // coefficients [4q, 4q + 4)
        int l[4][3];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int i = 4 * q + e;
            const int v = i < ea.n_words ? (int)(signed char)ea.data[(long)i * ea.ws + w] : 0;   // (zero padding, ram.rs:363-367)
            table_encode_value(v, ea.k_pt, ea.size_pt, l[e]);
        }
#pragma unroll
        for (int j = 0; j < S; j++) {
            reinterpret_cast<int4*>(rp + glwe_off(j, 0))[q] = make_int4(l[0][j], l[1][j], l[2][j], l[3][j]);
            reinterpret_cast<int4*>(rp + glwe_off(j, 1))[q] = make_int4(0, 0, 0, 0);
        }
    }
}

void table_fan_launch(int n_ct, hipStream_t stream, const TableFanArgs& fa) {
    hipLaunchKernelGGL(k_table_fan, dim3(1, n_ct, TABLE_SLICES), dim3(256), 0, stream, fa);
}
void table_encode_launch(int ws, hipStream_t stream, const TableEncodeArgs& ea) {
    hipLaunchKernelGGL(k_table_encode, dim3(1, ws, TABLE_SLICES), dim3(256), 0, stream, ea);
}

}  // namespace fk
