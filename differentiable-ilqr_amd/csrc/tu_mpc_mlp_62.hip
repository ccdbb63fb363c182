// tu_mpc_mlp_62.hip — the fused iteration and the one-launch small-batch solve
// on the one-hidden-layer network (dilqr_mlp_fused.h) instantiated for
// (n, m) = (6, 2): sigmoid and relu, the three bounds modes.
#include "dilqr_mlp_fused.h"

DILQR_MLP_FUSED_UNIT(6, 2)
