// The gradient of the masked L1 terms of the loss (dpt_runner.py:213, 228-229, 239-243) in one place: the loss kernel (train_opt.hip)
// and the compositor launches that form the same gradients on the spot (rays.hip, train_rays.hip) must agree bit for bit.
// The expression has no mul + add pair, so the including file's contraction setting cannot change it.
#pragma once
#include "vdn_common.h"

namespace vdn {

// d / d x of |x - gt| * m / mask_sum, e = (x - gt) * m; the caller multiplies by its weights behind it
VDN_DEV float l1_grad(float e, float m, float mask_sum) {
    const float sgn = e > 0.0f ? 1.0f : (e < 0.0f ? -1.0f : 0.0f);
    return sgn * m / mask_sum;
}
// mask_sum of a step without a mask (mask = ones over the B rays)
VDN_DEV float mask_sum_of_ones(int B) { return (float)B + 1e-5f; }

}  // namespace vdn
