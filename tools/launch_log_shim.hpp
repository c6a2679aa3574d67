// tools/launch_log.hip: what this tree's csrc/ has no name for.  read_top's fuse_ep and gated ask whether the final trace over Y
// ciphertexts takes the tail launch (path.hpp read_top, tail_top).
namespace { bool shim_tail_top(const fheram_ctx* c, int Y) { return chain_form(c, ChainQuery{false, LOGN, 1, Y}).form == ChainForm::Tail; } }
