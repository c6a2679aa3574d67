// k_select_pack_lanes: packed[y] = glwe_normalize( sum_{j < m} X^j * table[y][j] ) for every output ciphertext y = k * ws + w of a
// fheram_bank_select_lanes call (select k, word ciphertext w) as ONE launch.  table[y][j] is ONE ciphertext: GLWE `lane` of the source word that
// lane (k, j, w) names, so a candidate is assembled byte by byte (the store merge's "SB at offset 1" is [y0, x0, y2, y3]); a null pointer is the
// all-zero ciphertext and is skipped.  The arithmetic is k_select_pack's (select_pack.hip):
//   rotation       : the negacyclic index shift with its sign flip (rot_src / cneg)
//   sum            : int32 — at most 32 limbs of magnitude <= 2^16 are below 2^22
//   normalisation  : one carry pass over the 3 limbs from the least significant one (normalize_coeff<3, 3>)
// The table is read with wave-uniform loads (the index is blockIdx.y and the loop counter), and ONCE per workgroup and candidate: the loop over
// the candidates is the outer one, each thread keeping the sums of its 4 coefficients in registers.  Plain vector loads and stores only.
// A translation unit of its own (select_lanes.hpp says why).
#undef FK_STAMP
#define FK_NO_PLAIN_KERNELS
#include "kernels.hpp"
#include "select_lanes.hpp"

namespace fk {

constexpr int LANES_PER = 2 * N / (256 * SELECT_LANES_SLICES);   // coefficients of a thread
static_assert(LANES_PER * 256 * SELECT_LANES_SLICES == 2 * N, "the workgroups of an output ciphertext cover its 2N coefficients exactly");

__global__ __launch_bounds__(256) void k_select_pack_lanes(SelectLanesArgs sa) {
    constexpr int S = 3;
    const int y = (int)blockIdx.y, k = y / sa.ws;
    const int32_t* const* tab = sa.table + (long)y * SELECT_CAND_MAX;
    int32_t* op = sa.out + (long)y * (S * 2 * N);
    const int m = sa.m[k];
    const int base = (int)blockIdx.z * (256 * LANES_PER) + (int)threadIdx.x;   // coefficient q of the thread: base + 256 * q, < 2N
    int acc[LANES_PER][S];
#pragma unroll
    for (int q = 0; q < LANES_PER; q++)
#pragma unroll
        for (int l = 0; l < S; l++) acc[q][l] = 0;
    for (int j = 0; j < m; j++) {
        const int32_t* cp = tab[j];   // (uniform: one load per workgroup and candidate)
        if (!cp) continue;
#pragma unroll
        for (int q = 0; q < LANES_PER; q++) {
            const int idx = base + 256 * q, col = idx >> LOGN, i = idx & (N - 1);
            int src; bool sgn;
            rot_src(i, j, src, sgn);
#pragma unroll
            for (int l = 0; l < S; l++) acc[q][l] += cneg(cp[glwe_off(l, col) + src], sgn);
        }
    }
#pragma unroll
    for (int q = 0; q < LANES_PER; q++) {
        const int idx = base + 256 * q, col = idx >> LOGN, i = idx & (N - 1);
        double in_l[S], out_l[S];
#pragma unroll
        for (int l = 0; l < S; l++) in_l[l] = (double)acc[q][l];
        normalize_coeff<S, S>(in_l, out_l);
#pragma unroll
        for (int l = 0; l < S; l++) op[glwe_off(l, col) + i] = (int)out_l[l];
    }
}

void select_lanes_launch(int n_ct, hipStream_t stream, const SelectLanesArgs& sa) {
    hipLaunchKernelGGL(k_select_pack_lanes, dim3(1, n_ct, SELECT_LANES_SLICES), dim3(256), 0, stream, sa);
}

}  // namespace fk
