// k_cmux_chain (cmux_chain.hip): Address::set_from_fheuint for K encrypted integers as ONE launch — what fheram.hip sees of it.
// The kernel lives in a translation unit of its own: compiled into fheram.hip's, it changed the register counts of two unrelated kernels
// (the limb-split steps of the GGSW inversion), and DESIGN.md 10.3 wants a change of an existing kernel's code to be a measured decision.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fk {

constexpr int DERIVE_K_MAX = 8, DERIVE_DIGITS_MAX = 8;
struct CmuxChainArgs {                    // by value: no table in device memory
    const double* fu[DERIVE_K_MAX];       // integer k, prepared: [n_bits] GGSW (5 limbs, dnum 4)
    int32_t* out[DERIVE_K_MAX];           // address k's digits: [n_digits] GGSW (4 limbs, dnum 3)
    const double* tw;                     // the context's twiddle table (with the round-off monitor's words)
    unsigned char first[DERIVE_DIGITS_MAX], bits[DERIVE_DIGITS_MAX], lsh[DERIVE_DIGITS_MAX];   // the digit plan: bit_rsh, bit_mask, bit_lsh of conversion.rs:45-62
    int sign;
};
// the kernel's dynamic LDS (what LDSATTR does for the kernels of fheram.hip)
hipError_t cmux_chain_register();
// grid: (6 rows of a digit, n_digits, K)
void cmux_chain_launch(dim3 grid, hipStream_t stream, const CmuxChainArgs& ca);

}  // namespace fk
