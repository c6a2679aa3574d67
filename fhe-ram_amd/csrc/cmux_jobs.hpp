// k_cmux_jobs (cmux_jobs.hip): the CMux chains of Address::set_from_fheuint as a FLAT LIST OF DIGIT JOBS in ONE launch — what fheram.hip sees
// of it.  k_cmux_chain (cmux_chain.hpp) takes one digit plan for all its integers; here every output digit brings its own integer, first bit,
// width, shift and sign, so the addresses, selectors and selector fields of a whole step are one launch (fheram_bank_derive_list).
// A translation unit of its own, as every kernel since k_cmux_chain: the device code of every other kernel stays as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fk {

constexpr int CMUX_JOBS_MAX = 64;
struct CmuxJob {                  // one output digit
    const double* fu;             // the integer, prepared: [n_bits] GGSW (5 limbs, dnum 4)
    int32_t* out;                 // this digit's 6 rows: one GGSW (4 limbs, dnum 3)
    unsigned char first, bits, lsh, sign;   // bit_rsh, bit_mask, bit_lsh of conversion.rs:45-62; sign != 0: X^+v
};
struct CmuxJobsArgs {             // by value (about 1.5 KB): no table in device memory
    CmuxJob job[CMUX_JOBS_MAX];
    const double* tw;             // the context's twiddle table (with the round-off monitor's words)
};
// the kernel's dynamic LDS (what LDSATTR does for the kernels of fheram.hip)
hipError_t cmux_jobs_register();
// grid: (6 rows of a digit, n_jobs)
void cmux_jobs_launch(int rows, int n_jobs, hipStream_t stream, const CmuxJobsArgs& ja);

}  // namespace fk
