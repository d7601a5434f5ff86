// The launcher of the run-time-shaped convolution family (conv_any.hip), for conv.hip: the entries, the plan's record and the reducers stay there.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_dispatch.h"

namespace piso {

// Launches the main kernel of a CF_FWD_ANY / CF_WG_ANY plan - b: w_laid_out [ks][ks][CINP4][COUTP] (forward) / grad_out (weight gradient);
// out: `out` (forward) / the band partials [band][ks][ks][CINP16][COUTP] (weight gradient, which conv.hip then reduces).  PISO_OK or the launch error.
int conv_any_launch(const ConvPlan& p, const float* in, const float* b, float* out, hipStream_t stream);

}  // namespace piso
