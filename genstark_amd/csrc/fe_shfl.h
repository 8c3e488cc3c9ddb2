// fe_shfl.h — a field element moved between the lanes of a wave, limb by limb: shared by the batch inversion (pointwise.hip) and the
// scans (scan.hip).  Include after common.h.
#pragma once

__device__ __forceinline__ fe fe_shfl_up(const fe &v, int d) {
    fe o;
#pragma unroll
    for (int l = 0; l < GF_LIMBS; l++) fe_set_limb(o, l, __shfl_up(fe_limb(v, l), d));
    return o;
}
__device__ __forceinline__ fe fe_shfl_down(const fe &v, int d) {
    fe o;
#pragma unroll
    for (int l = 0; l < GF_LIMBS; l++) fe_set_limb(o, l, __shfl_down(fe_limb(v, l), d));
    return o;
}
__device__ __forceinline__ fe fe_shfl(const fe &v, int lane) {
    fe o;
#pragma unroll
    for (int l = 0; l < GF_LIMBS; l++) fe_set_limb(o, l, __shfl(fe_limb(v, l), lane));
    return o;
}
