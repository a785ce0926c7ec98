// The dropout instantiations of the fused LeNet-5 head (mlp_head_k with a HeadDrop closing its
// argument pack, with and without label smoothing) and their launcher, compiled from mlp_head.hip's
// kernel text as a translation unit -- and so a code object -- of their own: see the note at
// MNISTX_HEAD_SMOOTH_TU there.
#define MNISTX_HEAD_DROP_TU 1
#include "mlp_head.hip"
