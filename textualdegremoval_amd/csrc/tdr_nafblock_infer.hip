// Forward-only NAFBlock chains: tdr_naf_tail_infer / tdr_naf_head_infer, the KEEP = false instantiations of the kernels in
// tdr_nafblock.hip (same tiles, waves, MFMA sequence and reduction order; the stores of the tensors only a backward pass reads are
// compiled out).  A translation unit of its own: the object of tdr_nafblock.hip holds the training kernels alone, as it did.
#define TDR_NAF_INFER_TU 1
#include "tdr_nafblock.hip"
