// k_cmux_chain: Address::set_from_fheuint (conversion.rs:41-65) for K encrypted integers as ONE launch (fheram_address_derive).
// One workgroup per output GGSW row: grid (6 rows of a digit, n_digits, K).  The digits of an address are independent of each other, and
// inside a digit each of the DNUM_CT * 2 rows is a chain of its own of one CMux step per bit of the digit, so a workgroup never needs
// another workgroup's data: no counters, nothing that waits.  A workgroup whose digit has fewer bits ends earlier.
//   row       <- the noiseless gadget row (1 at coefficient 0 of limb r; body for col_in 0, mask column for col_in 1), written by the workgroup
//   per bit i:   row <- normalize(row + normalize(X^(+-2^(i + lsh)) row - row) (x) GGSW(b_(first + i)))
// with the arithmetic of k_cmux_pre, k_ext_product_fine<4, 5> + k_ext_product_fine_norm<4, 5> and k_add_norm (setup.hpp: the unchanged
// fheram_address_set_from_fheuint), except that the 8 terms of an output limb are accumulated in the transform domain and inverted ONCE:
// under the exactness contract (fft_dev.hpp: 8 terms of 17-bit limbs < 2^47, round-off below 1/2 — checked by the monitor) the rounded sum
// is the sum of the rounded terms.  The two carry chains of a step (the product's 5 -> 4 limbs, then row + product) both run from the least
// significant limb upwards, so they run side by side and each output limb is stored once.
// Between steps the row goes through its own slot of the address's digit buffer (nobody else touches it), behind a __syncthreads().
// Registers: the 2 * 4 transformed input limbs stay in registers (128); the operands are fetched two polynomials at a time.
// A translation unit of its own (cmux_chain.hpp says why); the argument struct and the two host entry points are declared there.
#undef FK_STAMP   // (the stamp buffer of the diagnostic build belongs to fheram.hip)
#define FK_NO_PLAIN_KERNELS
#include "kernels.hpp"
#include "cmux_chain.hpp"

namespace fk {

#include "cmux_step.inc"

template <int SA, int SG>
__global__ __launch_bounds__(T, T / 256) void k_cmux_chain(CmuxChainArgs ca) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    RoMonitor ro_mon(lds, ca.tw);
    double* tw = lds;
    double* data = lds + LDS_TW;
    const int row = (int)blockIdx.x, dig = (int)blockIdx.y, kk = (int)blockIdx.z;
    int32_t* acc = ca.out[kk] + ((long)dig * (int)gridDim.x + row) * (SA * 2 * N);
    const double* fu = ca.fu[kk];
    const int nb = ca.bits[dig], b0 = ca.first[dig], lsh = ca.lsh[dig];
    {   // test_vector = X^0 on gadget row r = row / 2 (conversion.rs:42-43): body limb r for col_in 0, mask limb r for col_in 1, i.e. polynomial r * 2 + col_in = row
        const int t0 = vt((int)threadIdx.x);
#pragma unroll
        for (int p = 0; p < SA * 2; p++)
#pragma unroll
            for (int k = 0; k < E; k++) acc[(long)p * N + t0 + T * k] = (p == row && t0 == 0 && k == 0) ? 1 : 0;
        load_twiddles(tw, ca.tw, t0);   // (ends with a __syncthreads: the row is written)
    }
#pragma unroll 1
    for (int i = 0; i < nb; i++) {
        int tid = vt((int)threadIdx.x);
        asm volatile("" : "+v"(tid));   // see k_ext_product_chain
        __builtin_assume(tid >= 0 && tid < T);
        const int step = 1 << (i + lsh);
        cmux_step<SA, SG>(acc, fu + (long)(b0 + i) * (SA * 2 * SG * 2 * N), ca.sign ? step : -step, tw, data, tid);
        __syncthreads();   // the step's stores have completed and its LDS traffic is over
    }
}

hipError_t cmux_chain_register() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cmux_chain<4, 5>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
}
void cmux_chain_launch(dim3 grid, hipStream_t stream, const CmuxChainArgs& ca) {
    hipLaunchKernelGGL((k_cmux_chain<4, 5>), grid, dim3(T), LDS_BYTES, stream, ca);
}

}  // namespace fk
