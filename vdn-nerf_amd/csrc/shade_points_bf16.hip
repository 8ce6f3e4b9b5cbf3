// Vertex shading of a mesh in one launch (k_sdf_fwd2.h MODE 4): SDFNetwork.forward + .gradient (fields.py:72-108) and the colour head
// (fields.py:148-176) on free-standing points, each seen straight down its own normal.
// (built with -fno-slp-vectorize -mllvm -amdgpu-mfma-vgpr-form=1 like sdf_bf16.hip, vdn_hip/build.py)
#include "k_sdf_fwd2.h"

extern "C" int vdn_shade_points_bf16(const VdnSdfArgs* sa, const void* color_blob, int32_t squeeze_out, float* col_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (sa == nullptr || color_blob == nullptr || col_out == nullptr || sa->blob == nullptr || sa->P <= 0) return -1;
    if (sa->pts == nullptr) return -2;
    if (sa->sdf == nullptr || sa->normals == nullptr) return -3;
    // (saves, a work list and the tail split belong to the training forward: the separate launches take them)
    if (sa->H != nullptr || sa->V != nullptr || sa->PE != nullptr || sa->U_pe != nullptr || sa->feat != nullptr || sa->active_idx != nullptr ||
        sa->n_active != nullptr || sa->tail_max_rows != 0) return -10;
    vdn::sdf2::ShadeExtra ex{};
    ex.color_blob = static_cast<const char*>(color_blob);
    ex.squeeze_out = squeeze_out;
    ex.col_out = col_out;
    return vdn::sdf2::launch<4, false, 4, 3>(sa, stream, nullptr, &ex);
}
