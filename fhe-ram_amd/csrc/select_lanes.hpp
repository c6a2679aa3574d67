// k_select_pack_lanes (select_lanes.hip): the pack of fheram_bank_select_lanes — what fheram.hip sees of it.
// As k_select_pack, with every candidate assembled lane by lane: output ciphertext y takes candidate j from its OWN pointer, so a candidate's
// byte w may be any byte of any source word.  Up to 64 x 32 pointers (16 KiB) do not fit kernel arguments: they are a table in device memory.
// A translation unit of its own, as k_select_pack and k_cmux_chain are (select_pack.hpp, cmux_chain.hpp): the device code of every other
// kernel stays exactly as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "select_pack.hpp"

namespace fk {

constexpr int SELECT_LANES_SLICES = 8;      // workgroups per output ciphertext (blockIdx.z): each thread owns 2N / (256 * 8) = 4 coefficients
constexpr int SELECT_LANES_CT_MAX = 64;     // output ciphertexts of one call (n * ws)
struct SelectLanesArgs {
    const int32_t* const* table;            // [n * ws][SELECT_CAND_MAX]: candidate j of output ciphertext y, ONE GLWE (3 limbs), the lane offset already applied; nullptr: zero
    int32_t* out;                           // [n * ws] GLWE: the packed rows
    int m[SELECT_K_MAX];                    // candidates of select k
    int ws;
};
// grid: (1, n_ct = n * ws, SELECT_LANES_SLICES)
void select_lanes_launch(int n_ct, hipStream_t stream, const SelectLanesArgs& sa);

}  // namespace fk
