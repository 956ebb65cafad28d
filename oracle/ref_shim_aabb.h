// Forced include for aabb_gpu.cu only: that file defines its own static float atomicMin / atomicMax, which collide with
// HIP's float overloads. Renaming them AFTER the HIP headers are in leaves HIP's declarations alone.
#pragma once
#include "ref_shim.h"
#define atomicMin refAtomicMin
#define atomicMax refAtomicMax
