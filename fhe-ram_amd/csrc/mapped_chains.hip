// k_read_chain_m / k_write_chain_m: the table forms of the row chains (kernels.hpp: k_read_chain_t / k_write_chain_t) with the member map
// applied wherever the chain reads OR writes rows — the source and the in-place products' store of read_prepare_write, ct_hi and the last
// product's store of write.  fheram_bank_read_prepare_write_list / fheram_bank_write_list launch them; every other operation launches the
// kernels it launched before.  A translation unit of its own (mapped_chains.hpp says why); the bodies are chain_kernels.inc and
// write_chain.inc, included by kernels.hpp a further time under FK_MAPPED_CHAINS.
#undef FK_STAMP   // (the stamp buffer of the diagnostic build belongs to fheram.hip)
#define FK_NO_PLAIN_KERNELS
#define FK_MAPPED_CHAINS
#include "mapped_chains.hpp"

namespace fk {

hipError_t mapped_chains_register() {
    const void* kernels[] = {reinterpret_cast<const void*>(&k_read_chain_m<4, 4>), reinterpret_cast<const void*>(&k_read_chain_m<5, 4>),
                             reinterpret_cast<const void*>(&k_write_chain_m<4, 4>), reinterpret_cast<const void*>(&k_write_chain_m<5, 4>)};
    for (const void* k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
void read_chain_m_launch(int sk, dim3 grid, hipStream_t stream, const RowChainTableArgs& ra) {
    if (sk == 5) hipLaunchKernelGGL((k_read_chain_m<5, 4>), grid, dim3(T), LDS_BYTES, stream, ra);
    else hipLaunchKernelGGL((k_read_chain_m<4, 4>), grid, dim3(T), LDS_BYTES, stream, ra);
}
void write_chain_m_launch(int sk, dim3 grid, hipStream_t stream, const RowChainTableArgs& ra) {
    if (sk == 5) hipLaunchKernelGGL((k_write_chain_m<5, 4>), grid, dim3(T), LDS_BYTES, stream, ra);
    else hipLaunchKernelGGL((k_write_chain_m<4, 4>), grid, dim3(T), LDS_BYTES, stream, ra);
}

}  // namespace fk
