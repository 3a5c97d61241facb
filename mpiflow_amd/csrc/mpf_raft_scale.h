// mpf_raft_scale.h - RAFT.forward's image scaling (RAFT/core/raft.py:89-90), shared by the kernels that build the feature network's batch
// (mpf_raft_glue.hip: k_raft_images; mpf_raft_eval.hip: k_raft_images_padded), so that a padded batch with no pad is the plain one, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// 2 * (x / 255) - 1 with a TRUE fp32 division (the library is built with the correctly rounded divide), as torch's CPU kernel computes it
__device__ __forceinline__ float raft_scale(float x) { return 2.0f * (x / 255.0f) - 1.0f; }
