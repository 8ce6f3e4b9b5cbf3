// bf16 instantiation of the background NeRF backward kernel - see k_nerf_bwd.h
#include "k_nerf_bwd.h"
extern "C" int vdn_nerf_mlp_bwd_bf16(const VdnNerfBwdArgs* args, void* stream) { return vdn::launch_nerf_bwd<vdn::BF16>(args, stream); }
extern "C" int vdn_nerf_mlp_bwd_input_bf16(const VdnNerfBwdArgs* args, const VdnNerfInputGradArgs* in, void* stream) {
    return vdn::launch_nerf_bwd_input<vdn::BF16>(args, in, stream);
}
