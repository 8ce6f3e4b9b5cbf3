// The per-ray tail of the ray generators (poses.py:189-212, dataset.py:111-118): the mask / colour / feature gathers of the
// pixel (x, y) from images resident in HBM, and near / far from the unit sphere. Shared by vdn_gen_rays (fixed poses) and
// vdn_gen_rays_pose (learnable poses) so that both write the same columns bit for bit.
#pragma once
#include "vdn_common.h"

namespace vdn {

template <class A>
VDN_DEV void gather_pixel_row(const A& a, float x, float y, float* o) {
    const int xi = min(max((int)x, 0), a.W - 1), yi = min(max((int)y, 0), a.H - 1);
    const long pix = (long)yi * a.W + xi;
    if (a.out_ld > 6) o[6] = a.mask ? a.mask[pix * a.mask_ch] : 1.0f;
    if (a.image != nullptr && a.out_ld >= 10) {
        o[7] = a.image[pix * 3];
        o[8] = a.image[pix * 3 + 1];
        o[9] = a.image[pix * 3 + 2];
    }
    if (a.feats != nullptr)
        for (int ch = 0; ch < a.C; ++ch) o[10 + ch] = a.feats[pix * a.C + ch];
}

// dataset.py:111-118 -> mid (near = mid - 1, far = mid + 1)
VDN_DEV float sphere_mid(const float* org, const float* d) {
    const float aa = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const float bb = 2.0f * (org[0] * d[0] + org[1] * d[1] + org[2] * d[2]);
    return 0.5f * (-bb) / aa;
}

}  // namespace vdn
