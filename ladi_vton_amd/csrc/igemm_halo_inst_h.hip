// Instantiation unit of the halo-resident 3x3 convolution kernel (igemm_halo_kernel.h): form group H of igemm_tiles.h.
#include "igemm_halo_kernel.h"
#include "igemm_tiles.h"
LADI_HALO_TILES_H(LADI_HALO_INSTANTIATE)
