// Forced include (-include) for compiling the reference's tf_ops/*.cu kernels and host launchers with hipcc.
// It maps names only: every cuda* spelling those files use onto its HIP equivalent. No arithmetic, no kernel text.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define cudaError_t hipError_t
#define cudaSuccess hipSuccess
#define cudaGetErrorString hipGetErrorString
#define cudaPeekAtLastError hipPeekAtLastError
#define cudaMalloc hipMalloc
#define cudaFree hipFree
#define cudaMemset hipMemset
#define cudaMemcpy hipMemcpy
#define cudaMemcpyHostToDevice hipMemcpyHostToDevice
#define cudaMemcpyDeviceToHost hipMemcpyDeviceToHost
#define cudaMemcpyDeviceToDevice hipMemcpyDeviceToDevice
// hipMemcpyToSymbol takes the symbol wrapped in HIP_SYMBOL
#define cudaMemcpyToSymbol(sym, ...) hipMemcpyToSymbol(HIP_SYMBOL(sym), __VA_ARGS__)
// only reached under PRINT_CONV_INFO, which the recipe never defines; kept so that the flag still compiles
#define cudaEvent_t hipEvent_t
#define cudaEventCreate hipEventCreate
#define cudaEventRecord(e) hipEventRecord((e), 0)
#define cudaEventSynchronize hipEventSynchronize
#define cudaEventElapsedTime hipEventElapsedTime
