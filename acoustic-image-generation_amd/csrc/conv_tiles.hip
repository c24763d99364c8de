// The one object that holds the 128x128 and 128x64 instances of igemm_f32_kernel, igemm_split3_kernel and igemm_split3d_kernel
// for gfx950: no host code, only the explicit instantiations of the list in conv_tiles.hpp (which says why they stay together).
#define ACIMG_TILE template __global__ void
#include "conv_tiles.hpp"
