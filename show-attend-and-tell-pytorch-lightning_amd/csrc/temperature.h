// Internal C++ entry points of temperature-scaling calibration (temperature.hip; wrapped by the C ABI in api.hip).
#pragma once
#include "common.h"

namespace sat {
constexpr int kMaxTemperatures = 8;
size_t temperature_workspace_bytes(int P, int V);
int temperature_nll(const float* logits, const int* targets, int P, int V, const float* temperatures, int n, float* loss_out, float* grad_out,
                    char* ws, hipStream_t st);
int temperature_fit(const float* logits, const int* targets, int P, int V, float init, float lr, float momentum, int nesterov, int iters,
                    float* t_trace, float* loss_trace, char* ws, hipStream_t st);
}  // namespace sat
