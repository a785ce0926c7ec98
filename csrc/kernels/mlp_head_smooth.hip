// The label-smoothing instantiations of the fused heads (mlp_head_k and ce_tail_k with SMOOTH set,
// eps as their one extra argument) and their launchers, compiled from mlp_head.hip's kernel text
// as a translation unit -- and so a code object -- of their own: see the note at
// MNISTX_HEAD_SMOOTH_TU there.
#define MNISTX_HEAD_SMOOTH_TU 1
#include "mlp_head.hip"
