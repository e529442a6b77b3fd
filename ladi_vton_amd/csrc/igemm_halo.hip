// Halo-resident 3x3 convolution (round 3): the eligibility tests of its three kinds of form (ring-halo, 2-D blocked, folded upsample).  The
// kernel and its launcher template live in igemm_halo_kernel.h; the nineteen forms are rows of igemm_tiles.h, compiled in the units
// igemm_halo_inst_{a..j}.hip and dispatched by base id from igemm.hip.
#include "common.h"
#include "kernels.h"
#include <algorithm>

namespace { constexpr int HALO_WMAX = 48; }

bool ladi_igemm_halo_eligible(const IGemmArgs& a, int batch) {
    return a.ksize == 3 && a.stride == 1 && a.pad == 1 && !a.ups && a.Ws <= HALO_WMAX && a.Ho == a.Hs && a.Wo == a.Ws && !(a.C0 % 64) && !(a.C1 % 64) &&
           batch == 1 && (size_t)a.P * (size_t)std::max(a.ld0, a.ld1) * 2 < 0x7FFFFFFFull;
}

// folded-upsample form (round 6): nearest-2x upsample + 3x3 convolution, single source, output rows of at most 48 pixels, whole `bp`-pixel tiles
// inside a sample
bool ladi_igemm_halo_ups_eligible(const IGemmArgs& a, int batch, int bp) {
    return a.ksize == 3 && a.stride == 1 && a.pad == 1 && a.ups == 1 && a.Ho == 2 * a.Hs && a.Wo == 2 * a.Ws && a.Wo <= HALO_WMAX && !a.C1 && !a.src1 &&
           !(a.C0 % 64) && batch == 1 && bp > 0 && !((a.Ho * a.Wo) % bp) && !(a.P % (a.Ho * a.Wo)) && (size_t)a.P * (size_t)a.ld0 * 2 < 0x7FFFFFFFull;
}

// 2-D blocked form: rows of any width that is a multiple of 32, whole blocks of `th` image rows
bool ladi_igemm_halo2d_eligible(const IGemmArgs& a, int batch, int th) {
    return a.ksize == 3 && a.stride == 1 && a.pad == 1 && !a.ups && a.Ho == a.Hs && a.Wo == a.Ws && !(a.C0 % 64) && !(a.C1 % 64) && batch == 1 &&
           !(a.Ws % 32) && th > 0 && !(a.Hs % th) && (size_t)a.P * (size_t)std::max(a.ld0, a.ld1) * 2 < 0x7FFFFFFFull;
}
