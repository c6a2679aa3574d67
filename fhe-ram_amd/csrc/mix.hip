// The kernels of fheram_bank_read_mix and fheram_bank_read_prepare_write_mix (mix.hpp): a read list, a table read and a register read
// of one bank — and the first halves of a member write list and of a register write — with ONE top.
//   k_trace_tail_x  the third inclusion of trace_tail.inc (FK_TAIL_TABLE 2): k_trace_tail_t with, per ciphertext, a source pointer (the
//                   packed row in the arena, the table's row, the register file's row: no gather launch), a pointer to its prepared digits
//                   and a product count of its own — 0 (a list entry of a one-coordinate bank: trace only) or 2 .. TAIL_EP_MAX.  A group
//                   is one ciphertext, its count is uniform within it, and groups never wait for each other.
//   k_read_chain_x  its predicated fallback: the further inclusion of chain_kernels.inc (FK_READ_CHAIN_TABLE 3), k_read_chain_t with the same
//                   three per-ciphertext arguments; a ciphertext without products leaves at once (k_keyswitch_chain redoes those).
//   k_mix_scatter   fheram_bank_read_prepare_write_mix's hand-over, ONE launch behind the top: run i copies ws GLWEs from src[i] to dst[i] —
//                   a prepared ciphertext's last product to the member's tree slot or the register file's row, its trace to the member's
//                   trtop / res slot or the register file's kept trace, a list read's result to its member's slot.  The elementwise
//                   kernels' slice geometry (MIX_SCATTER_SLICES workgroups of 256 threads per ciphertext), plain 16-byte vector loads and
//                   stores, no LDS.
// A translation unit of its own, as every kernel since k_cmux_chain (cmux_chain.hpp): compiled apart it leaves the device code of
// k_trace_tail, k_trace_tail_t, k_read_chain_t and of every other kernel exactly as it was.
#undef FK_STAMP   // (the stamp buffer of the diagnostic build belongs to fheram.hip)
#define FK_NO_PLAIN_KERNELS
#define FK_MIX_KERNELS_ONLY
#include "kernels.hpp"
#include "mix.hpp"

namespace fk {

static_assert(MIX_GROUPS == TAIL_GROUPS, "one ciphertext per group of the tail launch");

// this workgroup's ciphertext, as table_opnd_offset takes it: wave-uniform scalar work, recomputed where it is used
__device__ __forceinline__ int mix_row_y() {
    int y = (int)blockIdx.y;
    asm volatile("" : "+v"(y));
    return __builtin_amdgcn_readfirstlane(y);
}

#define FK_TAIL_NAME k_trace_tail_x
#define FK_TAIL_ARGS TailMixArgs
#define FK_TAIL_TABLE 2
#include "trace_tail.inc"
#undef FK_TAIL_NAME
#undef FK_TAIL_ARGS
#undef FK_TAIL_TABLE

#define FK_READ_CHAIN_ARGS RowChainMixArgs
#define FK_READ_CHAIN_TABLE 3
#define FK_READ_CHAIN_NAME k_read_chain_x
#define FK_VG FK_WIDE_VGPRS   // (as k_read_chain_t: a mix never runs beside the gate wave)
#include "chain_kernels.inc"
#undef FK_READ_CHAIN_NAME
#undef FK_VG
#undef FK_READ_CHAIN_ARGS
#undef FK_READ_CHAIN_TABLE

__global__ __launch_bounds__(256) void k_mix_scatter(MixScatterArgs sa) {
    constexpr int S = 3;
    const int i = (int)blockIdx.x;   // (uniform: the table is the launch's)
    const long ct = (long)blockIdx.y * (S * 2 * N);
    const int4* ap = reinterpret_cast<const int4*>(sa.src[i] + ct);
    int4* op = reinterpret_cast<int4*>(sa.dst[i] + ct);
    for (int idx = blockIdx.z * blockDim.x + threadIdx.x; idx < S * 2 * N / 4; idx += blockDim.x * gridDim.z) op[idx] = ap[idx];
}

hipError_t mix_register() {
    const void* kernels[] = {reinterpret_cast<const void*>(&k_trace_tail_x<3, 4, 3>), reinterpret_cast<const void*>(&k_trace_tail_x<3, 5, 3>),
                             reinterpret_cast<const void*>(&k_read_chain_x<4, 4>), reinterpret_cast<const void*>(&k_read_chain_x<5, 4>)};
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
void trace_tail_x_launch(int sk, hipStream_t stream, const TailMixArgs& ta) {
    if (sk == 5) hipLaunchKernelGGL((k_trace_tail_x<3, 5, 3>), dim3(TAIL_GROUPS * 2 * 5 * 3), dim3(T), LDS_BYTES, stream, ta);
    else hipLaunchKernelGGL((k_trace_tail_x<3, 4, 3>), dim3(TAIL_GROUPS * 2 * 4 * 3), dim3(T), LDS_BYTES, stream, ta);
}
void read_chain_x_launch(int sk, int n_ct, hipStream_t stream, const RowChainMixArgs& ra) {
    if (sk == 5) hipLaunchKernelGGL((k_read_chain_x<5, 4>), dim3(1, n_ct, 1), dim3(T), LDS_BYTES, stream, ra);
    else hipLaunchKernelGGL((k_read_chain_x<4, 4>), dim3(1, n_ct, 1), dim3(T), LDS_BYTES, stream, ra);
}
void mix_scatter_launch(int ws, hipStream_t stream, const MixScatterArgs& sa) {
    hipLaunchKernelGGL(k_mix_scatter, dim3(sa.n, ws, MIX_SCATTER_SLICES), dim3(256), 0, stream, sa);
}

}  // namespace fk
