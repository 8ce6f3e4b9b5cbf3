// f32 instantiation of the background NeRF backward kernel - see k_nerf_bwd.h
#include "k_nerf_bwd.h"
extern "C" int vdn_nerf_mlp_bwd_f32(const VdnNerfBwdArgs* args, void* stream) { return vdn::launch_nerf_bwd<vdn::F32>(args, stream); }
extern "C" int vdn_nerf_mlp_bwd_input_f32(const VdnNerfBwdArgs* args, const VdnNerfInputGradArgs* in, void* stream) {
    return vdn::launch_nerf_bwd_input<vdn::F32>(args, in, stream);
}
