// Forward-only NAFBlock chains: tdr_naf_tail_infer / tdr_naf_head_infer, the KEEP = false instantiations of the kernels in
// tdr_nafblock_chain.h (same tiles, waves, MFMA sequence and reduction order; the stores of the tensors only a backward pass reads are
// compiled out).  A translation unit of its own: next to the training kernels the compiler makes other code of these.
#include "tdr_nafblock_chain.h"

extern "C" int tdr_naf_tail_infer(const TdrNafTailDesc* d, void* stream) { return naf_tail_fwd_launch<false>(d, stream); }
extern "C" int tdr_naf_head_infer(const TdrNafHeadFwdDesc* d, void* stream) { return naf_head_fwd_launch<false>(d, stream); }
