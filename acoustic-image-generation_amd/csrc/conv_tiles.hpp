// The implicit-GEMM kernel instances that are compiled TOGETHER, in conv_tiles.hip, and only declared everywhere else.
//
// igemm_f32_kernel, igemm_split3_kernel and igemm_split3d_kernel end in the same igemm_epilogue<BM, BN, WGM, WGN, NTHR, TM, TN>
// (igemm_kernel.hpp).  For the 128x128 and 128x64 tiles all three instantiate it with the same arguments, and the code the
// compiler makes of that one function - it is specialised on what ALL its callers in a translation unit pass before it is
// inlined into each of them - depends on who else calls it: with the exact-f32, the on-the-fly and the trunk host code in
// three objects, these 18 kernels came out with other instruction streams than with all callers in one (the exact-f32 ones by
// about a thousand instructions each; tools/codeobj_diff.py, profiles/conv_host_split/).  So these instances are instantiated
// in ONE object, beside each other as they always were, and conv_f32.hip / conv_split.hip / conv_trunk.hip launch them
// through these declarations.  Every other instance (64x64, 256x16, 64x128, 128x32 tiles; every other kernel) has its
// epilogue to itself or was measured identical, and is instantiated by the file that launches it.
// A new 128x128 or 128x64 instance of one of the three kernels belongs in this list.
#pragma once
#include "igemm_split3d_kernel.hpp"      // (includes igemm_split3_kernel.hpp and igemm_kernel.hpp)

#ifndef ACIMG_TILE
#define ACIMG_TILE extern template __global__ void
#endif

namespace acimg {

ACIMG_TILE igemm_f32_kernel<128, 128, 2, 4, 512, false, false>(const IgemmParams);
ACIMG_TILE igemm_f32_kernel<128, 128, 2, 4, 512, false, true>(const IgemmParams);
ACIMG_TILE igemm_f32_kernel<128, 128, 2, 4, 512, true, false>(const IgemmParams);
ACIMG_TILE igemm_f32_kernel<128, 128, 2, 4, 512, true, true>(const IgemmParams);
ACIMG_TILE igemm_f32_kernel<128, 64, 2, 2, 256, false, false>(const IgemmParams);
ACIMG_TILE igemm_f32_kernel<128, 64, 2, 2, 256, false, true>(const IgemmParams);
ACIMG_TILE igemm_f32_kernel<128, 64, 2, 2, 256, true, false>(const IgemmParams);
ACIMG_TILE igemm_f32_kernel<128, 64, 2, 2, 256, true, true>(const IgemmParams);
ACIMG_TILE igemm_split3_kernel<128, 128, 2, 4, 512, SplitF16, 3>(const IgemmParams);
ACIMG_TILE igemm_split3_kernel<128, 128, 2, 4, 512, SplitBF16, 1>(const IgemmParams);
ACIMG_TILE igemm_split3_kernel<128, 128, 2, 4, 512, SplitBF16, 3>(const IgemmParams);
ACIMG_TILE igemm_split3_kernel<128, 64, 2, 2, 256, SplitF16, 3>(const IgemmParams);
ACIMG_TILE igemm_split3_kernel<128, 64, 2, 2, 256, SplitBF16, 1>(const IgemmParams);
ACIMG_TILE igemm_split3_kernel<128, 64, 2, 2, 256, SplitBF16, 3>(const IgemmParams);
ACIMG_TILE igemm_split3d_kernel<128, 128, 2, 4, 512, 2, 2, 3>(const IgemmParams);
ACIMG_TILE igemm_split3d_kernel<128, 128, 2, 4, 512, 2, 2, 1>(const IgemmParams);
ACIMG_TILE igemm_split3d_kernel<128, 64, 2, 2, 256, 2, 2, 3>(const IgemmParams);
ACIMG_TILE igemm_split3d_kernel<128, 64, 2, 2, 256, 2, 2, 1>(const IgemmParams);

}  // namespace acimg
