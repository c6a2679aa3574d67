// The three elementwise kernels of a bank's public side (public_io.hpp): plain loads, peek and poke at public addresses.
//   k_rows_plain   row x of word ciphertext w = the trivial ciphertext of byte w of words [x * N, (x + 1) * N) of the launch: mask limbs 0,
//                  body limbs encode_value's (setup.hpp; ram.rs:358-368) for a word below n_words and 0 behind — k_table_encode's rule
//                  (table.hip) over the rows of a member.  Integer arithmetic only.
//   k_peek_gather  out[y] = glwe_rotate(-q[y], *src[y]) for the n * ws chain inputs of a peek: source pointer and rotation per ciphertext in
//                  the argument struct.  Aligned 16-byte stores; the rotated reads are one dword each (q is any coefficient).
//   k_poke_merge   R[w] = glwe_normalize(R[w] - sum_j glwe_rotate(+q_j, t_j[w]) + sum_j glwe_rotate(+q_j, w_j[w])) over the entries j of the
//                  touched row, in place: write_first_step (ram.rs:574-576) with every term of the row in one pass.  The limb arithmetic
//                  is k_sub_add_norm<3>'s: the int32 sum (at most 1 + 2 * 16 terms of 17 bits), then one carry pass over the 3 limbs from
//                  the least significant one (normalize_coeff).  A thread owns the four coefficients it reads and writes of R.
// All cover a ciphertext as the elementwise kernels do (PUB_SLICES workgroups of 256 threads).  Plain vector loads and stores only: no
// LDS, nothing that waits for another workgroup.
// A translation unit of its own, as k_regs_fan and k_table_fan are (regs.hip, table.hip): compiled apart it leaves the device code of
// every other kernel exactly as it was.
#undef FK_STAMP
#define FK_NO_PLAIN_KERNELS
#define FK_PUBLIC_KERNELS_ONLY
#include "kernels.hpp"
#include "public_io.hpp"

namespace fk {

// limb j of encode_value(v, k_pt, size_pt) (setup.hpp), j < size_pt: v * 2^-k_pt on the torus in balanced base-2^17 digits (as table.hip)
__device__ __forceinline__ void plain_encode_value(int v, int k_pt, int size_pt, int (&limbs)[3]) {
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

__global__ __launch_bounds__(256) void k_rows_plain(RowsPlainArgs ra) {
    constexpr int S = 3;
    const int x = (int)blockIdx.x, w = (int)blockIdx.y;
    int32_t* rp = ra.rows + (long)w * ra.w_stride + (long)x * (S * 2 * N);
    const long word0 = (long)x * N;
    for (int q = blockIdx.z * blockDim.x + threadIdx.x; q < N / 4; q += blockDim.x * gridDim.z) {   // coefficients [4q, 4q + 4)
        int l[4][3];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const long j = word0 + 4 * q + e;
            const int v = j < ra.n_words ? (int)(signed char)ra.data[j * ra.ws + w] : 0;   // (zero padding, ram.rs:363-367)
            plain_encode_value(v, ra.k_pt, ra.size_pt, l[e]);
        }
#pragma unroll
        for (int j = 0; j < S; j++) {
            reinterpret_cast<int4*>(rp + glwe_off(j, 0))[q] = make_int4(l[0][j], l[1][j], l[2][j], l[3][j]);
            reinterpret_cast<int4*>(rp + glwe_off(j, 1))[q] = make_int4(0, 0, 0, 0);
        }
    }
}

// sign * a[src] for the coefficients [4q, 4q + 4) of rot(a, rho), a one polynomial of N coefficients
__device__ __forceinline__ int4 rot_load4(const int32_t* a, int q, int rho) {
    int v[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        int src; bool sgn;
        rot_src(4 * q + e, rho, src, sgn);
        v[e] = cneg(a[src], sgn);
    }
    return make_int4(v[0], v[1], v[2], v[3]);
}

__global__ __launch_bounds__(256) void k_peek_gather(PeekGatherArgs ga) {
    constexpr int S = 3;
    const int y = (int)blockIdx.y;
    const int32_t* ap = ga.src[y];   // (uniform: the table is the launch's)
    const int rho = -ga.q[y];
    int32_t* op = ga.out + (long)y * (S * 2 * N);
    for (int idx = blockIdx.z * blockDim.x + threadIdx.x; idx < S * 2 * N / 4; idx += blockDim.x * gridDim.z) {
        const int poly = idx / (N / 4), q = idx % (N / 4);   // poly = limb * 2 + column (glwe_off)
        reinterpret_cast<int4*>(op + (long)poly * N)[q] = rot_load4(ap + (long)poly * N, q, rho);
    }
}

__global__ __launch_bounds__(256) void k_poke_merge(PokeMergeArgs ma) {
    constexpr int S = 3;
    const int g = (int)blockIdx.x, w = (int)blockIdx.y;
    int32_t* rp = ma.row[g] + (long)w * ma.w_stride;
    const int j0 = ma.first[g], j1 = ma.first[g + 1];   // (uniform)
    const long ct = (long)w * (S * 2 * N);
    for (int idx = blockIdx.z * blockDim.x + threadIdx.x; idx < 2 * N / 4; idx += blockDim.x * gridDim.z) {
        const int col = idx / (N / 4), q = idx % (N / 4);
        int4 acc[S];
#pragma unroll
        for (int l = 0; l < S; l++) acc[l] = reinterpret_cast<const int4*>(rp + glwe_off(l, col))[q];
        for (int j = j0; j < j1; j++) {
            const int32_t* tp = ma.t[j] + ct;
            const int32_t* wp = ma.w[j] ? ma.w[j] + ct : nullptr;
            const int rho = ma.q[j];
#pragma unroll
            for (int l = 0; l < S; l++) {
                const int4 tv = rot_load4(tp + glwe_off(l, col), q, rho);
                acc[l].x -= tv.x; acc[l].y -= tv.y; acc[l].z -= tv.z; acc[l].w -= tv.w;
                if (wp) {
                    const int4 wv = rot_load4(wp + glwe_off(l, col), q, rho);
                    acc[l].x += wv.x; acc[l].y += wv.y; acc[l].z += wv.z; acc[l].w += wv.w;
                }
            }
        }
        int out[S][4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            double in_l[S], out_l[S];
#pragma unroll
            for (int l = 0; l < S; l++) in_l[l] = (double)(e == 0 ? acc[l].x : e == 1 ? acc[l].y : e == 2 ? acc[l].z : acc[l].w);
            normalize_coeff<S, S>(in_l, out_l);
#pragma unroll
            for (int l = 0; l < S; l++) out[l][e] = (int)out_l[l];
        }
#pragma unroll
        for (int l = 0; l < S; l++) reinterpret_cast<int4*>(rp + glwe_off(l, col))[q] = make_int4(out[l][0], out[l][1], out[l][2], out[l][3]);
    }
}

void rows_plain_launch(int n_rows, hipStream_t stream, const RowsPlainArgs& ra) {
    hipLaunchKernelGGL(k_rows_plain, dim3(n_rows, ra.ws, PUB_SLICES), dim3(256), 0, stream, ra);
}
void peek_gather_launch(int n_ct, hipStream_t stream, const PeekGatherArgs& ga) {
    hipLaunchKernelGGL(k_peek_gather, dim3(1, n_ct, PUB_SLICES), dim3(256), 0, stream, ga);
}
void poke_merge_launch(int n_touched, int ws, hipStream_t stream, const PokeMergeArgs& ma) {
    hipLaunchKernelGGL(k_poke_merge, dim3(n_touched, ws, PUB_SLICES), dim3(256), 0, stream, ma);
}

}  // namespace fk
