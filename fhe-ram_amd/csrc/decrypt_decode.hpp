// k_decrypt_decode (decrypt_decode.hip): GLWE::decrypt and decode_coeff_i64 of ciphertexts that stay where they are on the device — what
// fheram.hip sees of it (bank_setup.hpp: fheram_bank_source_decrypt, fheram_bank_ram_decrypt, _regs_decrypt, _table_decrypt).
// The kernel lives in a translation unit of its own, as every kernel since cmux_chain.hip: compiled apart it leaves the device code of
// every other kernel exactly as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fk {

constexpr int DECRYPT_SRC_MAX = 64;    // ciphertexts named one by one (the word form: n * ws of fheram_bank_source_decrypt)
constexpr int DECRYPT_ROWS_MAX = 256;  // ciphertexts of one launch of the row form, as the encrypt side chunks them (setup.hpp)
struct DecryptDecodeArgs {             // by value: no table in device memory, nothing to stage
    const int32_t* src[DECRYPT_SRC_MAX];   // base == nullptr: ciphertext x of the launch is src[x], ONE GLWE (3 limbs), read only
    const int32_t* base;                   // else ciphertext x is base + x * GLWE
    const double* s_hat;                   // the prepared secret (k_prepare)
    const double* tw;                      // the context's twiddle table (with the round-off monitor's words)
    long long want[DECRYPT_SRC_MAX];       // has_want: what coefficient 0 of ciphertext x is expected to hold; else every coefficient's own decoded value
    int has_want;
    int k, k_pt;                           // the ciphertext's precision and the plaintext's: 3 limbs of k, value at 2^-(k_pt)
    int n_coef, n_coef_last;               // coefficients [0, n_coef) of every ciphertext are decoded; [0, n_coef_last) of the launch's last one
    int32_t* values;                       // [grid][n_coef]: the decoded values
    long long* max_diff;                   // [grid]: max |diff| over the ciphertext's decoded coefficients
    long long* diff;                       // [grid][n_coef] or nullptr: diff of every decoded coefficient (the word form)
};
// the kernel's dynamic LDS (what LDSATTR does for the kernels of fheram.hip)
hipError_t decrypt_decode_register();
// grid: (n_ct)
void decrypt_decode_launch(int n_ct, hipStream_t stream, const DecryptDecodeArgs& da);

}  // namespace fk
