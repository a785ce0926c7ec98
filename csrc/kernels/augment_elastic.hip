// The elastic-distortion form of the augmentation kernel (augment_elastic_images_k: augment.hip's
// image kernel with AUG_EL set -- the displacement field drawn, smoothed and added in LDS) and the
// two probes the tests read its draws and field through, compiled from augment.hip's kernel text
// as a translation unit -- and so a code object -- of their own: see the note at
// MNISTX_AUG_ELASTIC_TU there.
#define MNISTX_AUG_ELASTIC_TU 1
#include "augment.hip"
