// The project's counter-based hash: 32 random bits as a pure function of (seed, 64-bit counter, stream id).  One definition for the
// synthetic-volume generator (datapath.hip) and the noise stage of the intensity augmentation (intensity.hip); oracle/datapath.py
// (_mix32 / _synth_bits) restates it bit for bit in numpy.
// Stream ids in use: 0 and 1 the synthetic volumes (image, labels), 2 and 3 the intensity noise (DA_INTENSITY_STREAM_U1 / _U2,
// include/deepatlas_hip.h), 4 the crop sampler's draws (crop.hip).
#pragma once
#include <hip/hip_runtime.h>

#define DA_CROP_STREAM 4u

__device__ __forceinline__ unsigned int da_mix32(unsigned int x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned int da_synth_bits(unsigned int seed, unsigned long long i, unsigned int stream_id) {
    const unsigned int hi = (unsigned int)(i >> 32), lo = (unsigned int)i;
    return da_mix32(da_mix32(lo ^ da_mix32(seed + 0x9e3779b9u * hi)) + stream_id);
}
