// k_select_pack (select_pack.hip): the pack of fheram_bank_select — what fheram.hip sees of it.
// The kernel lives in a translation unit of its own, as k_cmux_chain does (cmux_chain.hpp): compiled apart it leaves the device code of
// every kernel of fheram.hip exactly as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fk {

constexpr int SELECT_K_MAX = 8, SELECT_CAND_MAX = 32;
struct SelectPackArgs {                                   // by value: no table in device memory, nothing to stage
    const int32_t* cand[SELECT_K_MAX][SELECT_CAND_MAX];   // candidate j of select k: ws GLWEs (3 limbs), word w at w * GLWE; nullptr: all-zero ciphertexts
    int32_t* out;                                         // [n * ws] GLWE: the packed rows
    int m[SELECT_K_MAX];                                  // candidates of select k
    int ws;
};
// grid: (1, n * ws, slices)
void select_pack_launch(dim3 grid, hipStream_t stream, const SelectPackArgs& sa);

}  // namespace fk
