// piplib_amd/csrc/pip_adv_h.hip -- group H: the lean kernel with four waves per tableau (pip_lean.h, NW = 4), the two largest
// row-capacity classes: the second lean launch of pipamd_batch_solve, over the tableaux the first one paused
#include "pip_lean.h"
PIP_LEAN4_CLASSES(PIP_LEAN4_DEFINE)
