// k_cmux_jobs: Address::set_from_fheuint (conversion.rs:41-65) for a flat list of output digits as ONE launch (fheram_bank_derive_list).
// One workgroup per output GGSW row: grid (6 rows of a digit, n_jobs).  A job is one digit with an integer, a first bit, a width, a shift and
// a sign of its own, so digits of different addresses, selectors and selector fields sit side by side; as in k_cmux_chain (cmux_chain.hip)
// a workgroup never needs another workgroup's data: no counters, nothing that waits, and a workgroup whose digit has fewer bits ends earlier.
//   row       <- the noiseless gadget row, written by the workgroup
//   per bit i:   row <- normalize(row + normalize(X^(+-2^(i + lsh)) row - row) (x) GGSW(b_(first + i)))       (cmux_step, cmux_step.inc)
// The step is k_cmux_chain's own text, the loop around it is k_cmux_chain's with the plan read per job: the digits are the same integers.
// The job's fields are read from the argument segment with an index that is blockIdx.y: workgroup-uniform loads.  Plain vector stores only.
// A translation unit of its own (cmux_jobs.hpp says why).
#undef FK_STAMP   // (the stamp buffer of the diagnostic build belongs to fheram.hip)
#define FK_NO_PLAIN_KERNELS
#include "kernels.hpp"
#include "cmux_jobs.hpp"

namespace fk {

#include "cmux_step.inc"

template <int SA, int SG>
__global__ __launch_bounds__(T, T / 256) void k_cmux_jobs(CmuxJobsArgs ja) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    RoMonitor ro_mon(lds, ja.tw);
    double* tw = lds;
    double* data = lds + LDS_TW;
    const int row = (int)blockIdx.x, jb = (int)blockIdx.y;   // (the host launches n_jobs <= CMUX_JOBS_MAX)
    int32_t* acc = ja.job[jb].out + (long)row * (SA * 2 * N);
    const double* fu = ja.job[jb].fu;
    const int nb = ja.job[jb].bits, b0 = ja.job[jb].first, lsh = ja.job[jb].lsh, sign = ja.job[jb].sign;
    {   // test_vector = X^0 on gadget row r = row / 2 (conversion.rs:42-43): polynomial r * 2 + col_in = row, as k_cmux_chain writes it
        const int t0 = vt((int)threadIdx.x);
#pragma unroll
        for (int p = 0; p < SA * 2; p++)
#pragma unroll
            for (int k = 0; k < E; k++) acc[(long)p * N + t0 + T * k] = (p == row && t0 == 0 && k == 0) ? 1 : 0;
        load_twiddles(tw, ja.tw, t0);   // (ends with a __syncthreads: the row is written)
    }
#pragma unroll 1
    for (int i = 0; i < nb; i++) {
        int tid = vt((int)threadIdx.x);
        asm volatile("" : "+v"(tid));   // see k_ext_product_chain
        __builtin_assume(tid >= 0 && tid < T);
        const int step = 1 << (i + lsh);
        cmux_step<SA, SG>(acc, fu + (long)(b0 + i) * (SA * 2 * SG * 2 * N), sign ? step : -step, tw, data, tid);
        __syncthreads();   // the step's stores have completed and its LDS traffic is over
    }
}

hipError_t cmux_jobs_register() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cmux_jobs<4, 5>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
}
void cmux_jobs_launch(int rows, int n_jobs, hipStream_t stream, const CmuxJobsArgs& ja) {
    hipLaunchKernelGGL((k_cmux_jobs<4, 5>), dim3(rows, n_jobs, 1), dim3(T), LDS_BYTES, stream, ja);
}

}  // namespace fk
