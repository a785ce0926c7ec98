// The two-label instantiations of the fused heads (mlp_head_k and ce_tail_k with labels2 and lam behind
// eps in their argument pack: mixup / CutMix, with dropout and without) and their launchers, compiled
// from mlp_head.hip's kernel text as a translation unit -- and so a code object -- of their own: see
// the note at MNISTX_HEAD_SMOOTH_TU there.
#define MNISTX_HEAD_MIX_TU 1
#include "mlp_head.hip"
