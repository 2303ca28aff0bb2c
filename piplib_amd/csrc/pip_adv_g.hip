// piplib_amd/csrc/pip_adv_g.hip -- group G: the lean bulk kernel's BIG flavour (pip_lean.h: one parameter, the big one),
// one instantiation per row-capacity class
#include "pip_lean.h"
PIP_LEAN_BIG_CLASSES(PIP_LEAN_BIG_DEFINE)
