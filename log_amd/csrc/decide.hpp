// decide.hpp -- host-side declarations of decide.hip (included by decide.hip and api.hip only)
#pragma once
#include "common.hpp"

size_t lr_decide_scratch_bytes(int p);
hipError_t lr_launch_decide_depth(int p, const lograst_decide_depth_args& a, void* scratch, hipStream_t s);
hipError_t lr_launch_decide_init(int p, const lograst_decide_init_args& a, void* scratch, hipStream_t s);
hipError_t lr_launch_child_radius_max(int num_points, int num_children, const int32_t* index_parent, const float* scaling,
                                      float scaling_decay, float* radius3d_max, hipStream_t s);
