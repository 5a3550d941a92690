// cuda_runtime.h of oracle/cuda_host_shim: the CUDA / OptiX names that the reference's ray-marching shader and the headers it
// pulls in mention, as ordinary host C++, so that g++ can compile that shader text unmodified (oracle/ref_march_probe.cpp,
// oracle/build_ref.sh).  TEST INFRASTRUCTURE ONLY.  Written from the CUDA C++ Programming Guide, the CUDA Math API reference, the
// OptiX 7 Programming Guide and the compiler's list of undeclared names - not from NVIDIA's headers.
//
// Two kinds of names live here:
//   * host-side API that the include chain only MENTIONS in inline code nobody calls (memory, arrays, texture objects, streams,
//     accel builds): bare declarations, never defined, never linked;
//   * device-side names that the marcher EXECUTES (tex1D / tex3D, min / max, __powf, __frcp_rn, __int_as_float, optixTrace and the
//     optixGet* accessors): declared here, defined in shim_device.cpp, which states the rule each one follows.
// The build force-includes this file (-include) and defines __CUDACC__ (so that gdt's vector types grow their float3 / int3
// constructors and gdt::min / max resolve to the global ones below) but NOT __NVCC__ (kernel launches stay compiled out).
#pragma once
#ifndef OVR_CUDA_HOST_SHIM_H
#define OVR_CUDA_HOST_SHIM_H

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#ifndef __CUDACC__
#define __CUDACC__ 1
#endif
#define __device__
#define __host__
#define __global__
#define __constant__
#define __forceinline__ inline
#define __align__(n) alignas(n)
#define CUDARTAPI

// ---- built-in vector types (Programming Guide, "Built-in Vector Types") ------------------------------------------------------
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct int4 { int x, y, z, w; };
struct uint2 { unsigned x, y; };
struct uint3 { unsigned x, y, z; };
struct uint4 { unsigned x, y, z, w; };
struct dim3 { unsigned x = 1, y = 1, z = 1; };
inline float2 make_float2(float x, float y) { return { x, y }; }
inline float3 make_float3(float x, float y, float z) { return { x, y, z }; }
inline float4 make_float4(float x, float y, float z, float w) { return { x, y, z, w }; }
inline int2 make_int2(int x, int y) { return { x, y }; }
inline int3 make_int3(int x, int y, int z) { return { x, y, z }; }
inline uint2 make_uint2(unsigned x, unsigned y) { return { x, y }; }
inline uint3 make_uint3(unsigned x, unsigned y, unsigned z) { return { x, y, z }; }
extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;

// ---- min / max with CUDA's semantics ------------------------------------------------------------------------------------------
// CUDA Math API, fminf / fmaxf (and the float overloads of min / max, which are defined through them): "if one argument is NaN,
// returns the numeric argument".  std::min(a, b) returns a when the comparison with a NaN is false, which is a different function:
// gdt's clamp(x, 0, 1) = min(1, max(0, x)) maps NaN to 0 only with the rule below, and the shader relies on that for the normal of
// a zero gradient.
inline float min(float a, float b) { return fminf(a, b); }
inline float max(float a, float b) { return fmaxf(a, b); }
inline double min(double a, double b) { return fmin(a, b); }
inline double max(double a, double b) { return fmax(a, b); }
#define OVR_SHIM_INT_MINMAX(T)                       \
  inline T min(T a, T b) { return b < a ? b : a; }   \
  inline T max(T a, T b) { return a < b ? b : a; }
OVR_SHIM_INT_MINMAX(int)
OVR_SHIM_INT_MINMAX(unsigned)
OVR_SHIM_INT_MINMAX(long)
OVR_SHIM_INT_MINMAX(unsigned long)
OVR_SHIM_INT_MINMAX(long long)
OVR_SHIM_INT_MINMAX(unsigned long long)
#undef OVR_SHIM_INT_MINMAX

// ---- device intrinsics the marcher executes (defined in shim_device.cpp, except the bit casts) --------------------------------
inline float __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }   // reinterpretation of the bits, Math API
inline int __float_as_int(float f) { int i; std::memcpy(&i, &f, 4); return i; }
float __frcp_rn(float x);
// glibc's <cmath> already declares an extern "C" __powf that is libm's powf: the intrinsic gets a name of its own
float ovr_shim_powf(float x, float y);
#define __powf ovr_shim_powf

typedef unsigned long long cudaTextureObject_t, cudaSurfaceObject_t; // here: the address of an OvrShimTexture (ovr_shim.h)
template<typename T> T tex1D(cudaTextureObject_t tex, float x);
template<typename T> T tex3D(cudaTextureObject_t tex, float x, float y, float z);
template<> float tex1D<float>(cudaTextureObject_t, float);
template<> float4 tex1D<float4>(cudaTextureObject_t, float);
template<> float tex3D<float>(cudaTextureObject_t, float, float, float);

// ---- host runtime API: mentioned, never called ---------------------------------------------------------------------------------
typedef int cudaError_t;
enum { cudaSuccess = 0 };
typedef struct CUstream_st* cudaStream_t;
typedef struct cudaArray* cudaArray_t;
typedef unsigned long long CUdeviceptr;
struct cudaChannelFormatDesc { int x, y, z, w, f; };
struct cudaExtent { size_t width, height, depth; };
struct cudaPitchedPtr { void* ptr; size_t pitch, xsize, ysize; };
struct cudaPos { size_t x, y, z; };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice, cudaMemcpyDefault };
enum cudaTextureReadMode { cudaReadModeElementType, cudaReadModeNormalizedFloat };
enum cudaTextureFilterMode { cudaFilterModePoint, cudaFilterModeLinear };
enum cudaTextureAddressMode { cudaAddressModeWrap, cudaAddressModeClamp, cudaAddressModeMirror, cudaAddressModeBorder };
enum cudaResourceType { cudaResourceTypeArray };
struct cudaResourceDesc { cudaResourceType resType; struct { struct { cudaArray_t array; } array; } res; };
struct cudaTextureDesc {
  cudaTextureAddressMode addressMode[3];
  cudaTextureFilterMode filterMode, mipmapFilterMode;
  cudaTextureReadMode readMode;
  int normalizedCoords, sRGB;
  float maxAnisotropy, mipmapLevelBias, minMipmapLevelClamp, maxMipmapLevelClamp;
  float borderColor[4];
};
struct cudaMemcpy3DParms { cudaArray_t srcArray; cudaPos srcPos; cudaPitchedPtr srcPtr; cudaArray_t dstArray; cudaPos dstPos; cudaPitchedPtr dstPtr; cudaExtent extent; cudaMemcpyKind kind; };
inline cudaExtent make_cudaExtent(size_t w, size_t h, size_t d) { return { w, h, d }; }
inline cudaPitchedPtr make_cudaPitchedPtr(void* p, size_t pitch, size_t xs, size_t ys) { return { p, pitch, xs, ys }; }
template<typename T> cudaChannelFormatDesc cudaCreateChannelDesc();
const char* cudaGetErrorString(cudaError_t);
cudaError_t cudaGetLastError();
cudaError_t cudaDeviceSynchronize();
cudaError_t cudaMemGetInfo(size_t*, size_t*);
cudaError_t cudaFree(void*);
cudaError_t cudaFreeAsync(void*, cudaStream_t);
cudaError_t cudaFreeArray(cudaArray_t);
cudaError_t cudaMalloc(void**, size_t);
cudaError_t cudaMallocAsync(void**, size_t, cudaStream_t);
cudaError_t cudaMallocArray(cudaArray_t*, const cudaChannelFormatDesc*, size_t, size_t = 0, unsigned = 0);
cudaError_t cudaMalloc3DArray(cudaArray_t*, const cudaChannelFormatDesc*, cudaExtent, unsigned = 0);
cudaError_t cudaMemset(void*, int, size_t);
cudaError_t cudaMemsetAsync(void*, int, size_t, cudaStream_t = 0);
cudaError_t cudaMemcpy(void*, const void*, size_t, cudaMemcpyKind);
cudaError_t cudaMemcpyAsync(void*, const void*, size_t, cudaMemcpyKind, cudaStream_t = 0);
cudaError_t cudaMemcpy3D(const cudaMemcpy3DParms*);
cudaError_t cudaMemcpyToArray(cudaArray_t, size_t, size_t, const void*, size_t, cudaMemcpyKind);
cudaError_t cudaMemcpy2DToArray(cudaArray_t, size_t, size_t, const void*, size_t, size_t, size_t, cudaMemcpyKind);
cudaError_t cudaArrayGetInfo(cudaChannelFormatDesc*, cudaExtent*, unsigned*, cudaArray_t);
cudaError_t cudaCreateTextureObject(cudaTextureObject_t*, const cudaResourceDesc*, const cudaTextureDesc*, const void*);
cudaError_t cudaDestroyTextureObject(cudaTextureObject_t);
cudaError_t cudaStreamSynchronize(cudaStream_t);
cudaError_t cudaStreamCreate(cudaStream_t*);
cudaError_t cudaStreamDestroy(cudaStream_t);

// ---- OptiX host API: mentioned, never called ------------------------------------------------------------------------------------
typedef unsigned long long OptixTraversableHandle;
typedef struct OptixDeviceContext_t* OptixDeviceContext;
typedef int OptixResult;
enum { OPTIX_SUCCESS = 0 };
#define OPTIX_SBT_RECORD_ALIGNMENT 16
#define OPTIX_SBT_RECORD_HEADER_SIZE 32
struct OptixAabb { float minX, minY, minZ, maxX, maxY, maxZ; };
struct OptixBuildInput { int type; char opaque[1024]; };
struct OptixAccelBuildOptions { unsigned buildFlags; int operation; char opaque[64]; };
struct OptixAccelBufferSizes { size_t outputSizeInBytes, tempSizeInBytes, tempUpdateSizeInBytes; };
struct OptixAccelEmitDesc { CUdeviceptr result; int type; };
enum { OPTIX_PROPERTY_TYPE_COMPACTED_SIZE = 1, OPTIX_BUILD_OPERATION_BUILD = 1, OPTIX_BUILD_FLAG_NONE = 0, OPTIX_BUILD_FLAG_ALLOW_COMPACTION = 2 };
OptixResult optixAccelComputeMemoryUsage(OptixDeviceContext, const OptixAccelBuildOptions*, const OptixBuildInput*, unsigned, OptixAccelBufferSizes*);
OptixResult optixAccelBuild(OptixDeviceContext, cudaStream_t, const OptixAccelBuildOptions*, const OptixBuildInput*, unsigned, CUdeviceptr, size_t,
                            CUdeviceptr, size_t, OptixTraversableHandle*, const OptixAccelEmitDesc*, unsigned);
OptixResult optixAccelCompact(OptixDeviceContext, cudaStream_t, OptixTraversableHandle, CUdeviceptr, size_t, OptixTraversableHandle*);
const char* optixGetErrorName(OptixResult);
const char* optixGetErrorString(OptixResult);

// ---- OptiX device API: the sliver the marcher uses (defined in shim_device.cpp) -------------------------------------------------
typedef unsigned OptixVisibilityMask;
enum { OPTIX_RAY_FLAG_NONE = 0, OPTIX_RAY_FLAG_DISABLE_ANYHIT = 1 };
void optixTrace(OptixTraversableHandle handle, float3 origin, float3 direction, float tmin, float tmax, float time, OptixVisibilityMask mask,
                unsigned flags, unsigned sbt_offset, unsigned sbt_stride, unsigned miss_index, unsigned& p0, unsigned& p1);
bool optixReportIntersection(float t, unsigned kind, unsigned a0, unsigned a1);
float optixGetRayTmin();
float optixGetRayTmax();
float3 optixGetWorldRayOrigin();
float3 optixGetWorldRayDirection();
float3 optixGetObjectRayOrigin();
float3 optixGetObjectRayDirection();
unsigned optixGetPayload_0();
unsigned optixGetPayload_1();
unsigned optixGetAttribute_0();
unsigned optixGetAttribute_1();
unsigned optixGetRayVisibilityMask();
CUdeviceptr optixGetSbtDataPointer();
void optixGetWorldToObjectTransformMatrix(float m[12]);
void optixGetObjectToWorldTransformMatrix(float m[12]);
uint3 optixGetLaunchIndex();

#endif // OVR_CUDA_HOST_SHIM_H
