// The distilled instantiations of the fused heads (mlp_head_k and ce_tail_k with a CeDistill as their
// argument pack: the soft target of a frozen teacher's logits at a temperature, ce_stats.h) and their
// launchers, compiled from mlp_head.hip's kernel text as a translation unit -- and so a code object -- of
// their own: see the note at MNISTX_HEAD_SMOOTH_TU there.
#define MNISTX_HEAD_DISTILL_TU 1
#include "mlp_head.hip"
