// The known-pixel rule of the whole-raster kernels (raster.hip, seam.hip): one definition, so that they cannot disagree.
#pragma once
#include <math.h>

#include "common.h"

struct RasterIn {
    const float* dem;
    const float* mask;     // may be null
    int use_nodata;
    float nodata;
};

// known: mask != 0 (if given), finite, and not the nodata value (if given)
__device__ __forceinline__ bool rs_known(const RasterIn& in, int64_t i, float& z) {
    z = in.dem[i];
    bool k = isfinite(z);
    if (in.mask) k = k && in.mask[i] != 0.f;
    if (in.use_nodata) k = k && z != in.nodata;
    return k;
}
