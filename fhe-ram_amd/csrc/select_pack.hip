// k_select_pack: packed[y] = glwe_normalize( sum_{j < m} X^j * c_j[y] ) for every output ciphertext y = k * ws + w of a fheram_bank_select
// call (select k, word w) as ONE launch.  The candidates are coefficient-0 ciphertexts [v, 0, .., 0]; X^j moves candidate j to coefficient
// j of the row a one-row RAM would hold (ram.rs:334-380 packs its bytes the same way), so the blind rotation by the selector and the
// trace behind this launch are Ram::read on that row.
//   rotation       : the negacyclic index shift with its sign flip (rot_src / cneg, as k_rotate)
//   sum            : int32 — at most 32 limbs of magnitude <= 2^16 are below 2^22
//   normalisation  : one carry pass over the 3 limbs from the least significant one (normalize_coeff, as k_sub_add_norm); the sum is NOT
//                    normalised without it (401 074 > 2^17 was seen for 8 candidates), and the products that follow expect normalised limbs
// A candidate that is a null pointer is the all-zero ciphertext and is skipped.  Plain vector loads and stores only.
// A translation unit of its own (select_pack.hpp says why).
#undef FK_STAMP
#define FK_NO_PLAIN_KERNELS
#include "kernels.hpp"
#include "select_pack.hpp"

namespace fk {

__global__ __launch_bounds__(256) void k_select_pack(SelectPackArgs sa) {
    constexpr int S = 3;
    const int y = (int)blockIdx.y, k = y / sa.ws, w = y - k * sa.ws;
    const long word = (long)w * (S * 2 * N);
    int32_t* op = sa.out + (long)y * (S * 2 * N);
    const int m = sa.m[k];
    for (int idx = blockIdx.z * blockDim.x + threadIdx.x; idx < 2 * N; idx += blockDim.x * gridDim.z) {
        const int col = idx >> LOGN, i = idx & (N - 1);
        int acc[S];
#pragma unroll
        for (int l = 0; l < S; l++) acc[l] = 0;
        for (int j = 0; j < m; j++) {
            const int32_t* cp = sa.cand[k][j];
            if (!cp) continue;   // (uniform: the table is the launch's)
            int src; bool sgn;
            rot_src(i, j, src, sgn);
#pragma unroll
            for (int l = 0; l < S; l++) acc[l] += cneg(cp[word + glwe_off(l, col) + src], sgn);
        }
        double in_l[S], out_l[S];
#pragma unroll
        for (int l = 0; l < S; l++) in_l[l] = (double)acc[l];
        normalize_coeff<S, S>(in_l, out_l);
#pragma unroll
        for (int l = 0; l < S; l++) op[glwe_off(l, col) + i] = (int)out_l[l];
    }
}

void select_pack_launch(dim3 grid, hipStream_t stream, const SelectPackArgs& sa) {
    hipLaunchKernelGGL(k_select_pack, grid, dim3(256), 0, stream, sa);
}

}  // namespace fk
