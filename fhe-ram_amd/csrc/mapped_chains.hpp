// k_read_chain_m / k_write_chain_m (mapped_chains.hip): the row chains of a bank's read_prepare_write / write LIST, which read AND store
// the rows through the member map (kernels.hpp RowChainTableArgs) — what fheram.hip sees of them.
// The kernels live in a translation unit of their own, as k_cmux_chain does (cmux_chain.hpp): the mapped store costs k_read_chain_t<4, 4>
// forty spilled registers when it is added to that kernel, so the lists have instantiations of their own, and compiled
// apart they leave the device code of every kernel a range, a batch, a read list or a plain context launches exactly as it was.
#pragma once
#include "kernels.hpp"

namespace fk {

// the kernels' dynamic LDS (what LDSATTR does for the kernels of fheram.hip)
hipError_t mapped_chains_register();
// sk: the limb count of the context's trace keys (4 or 5); grid: (rows, n * ws)
void read_chain_m_launch(int sk, dim3 grid, hipStream_t stream, const RowChainTableArgs& ra);
void write_chain_m_launch(int sk, dim3 grid, hipStream_t stream, const RowChainTableArgs& ra);

}  // namespace fk
