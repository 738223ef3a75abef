// cuda_host.h -- a host execution layer for CUDA C translation units (test infrastructure).
//
// Written from the public semantics of the CUDA programming model; it holds nothing of any
// program compiled against it.  A .cu file whose launches were rewritten into
// cuda_host::launch(grid, block, has_barrier, [&]{ kernel(args); }) (oracle/cuda_host/rewrite.py)
// and that is compiled with `-include cuda_host.h` runs its kernels on the CPU:
//   * the address-space qualifiers are empty; __shared__ is `static`, so the threads of a
//     block, which run one block after another on one OS thread, share the block's arrays;
//   * a kernel without a barrier is a plain loop over its threads; a kernel with one runs every
//     thread of the block as a cooperative context of its own, and __syncthreads() returns once
//     every thread that has not yet left the kernel stands at a barrier (cuda_host.cpp);
//   * texture fetches from linear memory return 0 outside the bound range without reading
//     there, and are counted (cuda_host::stats), so a stage that leans on that is visible;
//   * device functions map onto libm.  The fast-math intrinsics (__fdividef, __sincosf, rsqrt)
//     are the exactly rounded operations here; CUDA's own error bounds are modelled elsewhere
//     (oracle/perturb.h), not in this layer.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>

#define __global__
#define __device__
#define __host__
#define __constant__
#define __shared__ static
#define __syncthreads() cuda_host::syncthreads()

// ------------------------------------------------------------------------------- vector types
struct uint3 { unsigned x, y, z; };
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct int4 { int x, y, z, w; };
struct uint4 { unsigned x, y, z, w; };
static inline float2 make_float2(float x, float y) { return float2{x, y}; }
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
static inline int3 make_int3(int x, int y, int z) { return int3{x, y, z}; }
static inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }

extern uint3 threadIdx, blockIdx;
extern dim3 blockDim, gridDim;

// ---------------------------------------------------------------------------- device functions
static inline int __mul24(int a, int b) { return a * b; }
static inline float __fdividef(float a, float b) { return a / b; }
// glibc declares a function of the intrinsic's name; the kernels get this one.
static inline void cuda_host_sincosf(float x, float* s, float* c) { *s = sinf(x); *c = cosf(x); }
#define __sincosf(x, s, c) cuda_host_sincosf(x, s, c)
static inline float rsqrt(float x) { return 1.0f / sqrtf(x); }
static inline float saturate(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
static inline float __int_as_float(int v) { float f; memcpy(&f, &v, 4); return f; }
static inline float __uint_as_float(unsigned v) { float f; memcpy(&f, &v, 4); return f; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline int min(int a, int b) { return a < b ? a : b; }
static inline unsigned max(unsigned a, unsigned b) { return a > b ? a : b; }
static inline unsigned min(unsigned a, unsigned b) { return a < b ? a : b; }
static inline float max(float a, float b) { return fmaxf(a, b); }
static inline float min(float a, float b) { return fminf(a, b); }
static inline double max(double a, double b) { return fmax(a, b); }
static inline double min(double a, double b) { return fmin(a, b); }
static inline double max(float a, double b) { return fmax((double)a, b); }
static inline double min(float a, double b) { return fmin((double)a, b); }
static inline double max(double a, float b) { return fmax(a, (double)b); }
static inline double min(double a, float b) { return fmin(a, (double)b); }

// ------------------------------------------------------------------------------------ runtime
typedef int cudaError_t;
typedef void* cudaStream_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost,
                      cudaMemcpyDeviceToDevice };
enum cudaChannelFormatKind { cudaChannelFormatKindSigned, cudaChannelFormatKindUnsigned,
                             cudaChannelFormatKindFloat };
enum cudaTextureReadMode { cudaReadModeElementType, cudaReadModeNormalizedFloat };
enum cudaTextureFilterMode { cudaFilterModePoint, cudaFilterModeLinear };
enum cudaTextureAddressMode { cudaAddressModeWrap, cudaAddressModeClamp };
struct cudaChannelFormatDesc { int x, y, z, w; cudaChannelFormatKind f; };
struct cudaArray;
struct cudaDeviceProp { int major, minor; size_t totalGlobalMem; char name[256]; };

// Defaults of a texture reference in CUDA: point sampling, unnormalised coordinates, clamping.
struct textureReference {
    int normalized = 0;
    cudaTextureFilterMode filterMode = cudaFilterModePoint;
    cudaTextureAddressMode addressMode[3] = {cudaAddressModeClamp, cudaAddressModeClamp,
                                             cudaAddressModeClamp};
    cudaChannelFormatDesc channelDesc = {0, 0, 0, 0, cudaChannelFormatKindFloat};
    const void* ptr = nullptr;   // bound linear memory
    size_t bytes = 0;            // 1D: bound size
    int width = 0, height = 0;   // 2D (bound with a pitch)
    size_t pitch = 0;
};
template <class T, int DIM = 1, cudaTextureReadMode MODE = cudaReadModeElementType>
struct texture : textureReference {};

namespace cuda_host {
struct Stats {
    long launches;      // kernel launches since reset
    long blocks;        // blocks run
    long oob_fetches;   // 1D fetches outside the bound range (returned 0), all launches
    long clamped_2d;    // 2D fetches whose coordinate was clamped to the edge
    long last_oob;      // the same two counts for the latest launch alone
    long last_clamped;
};
extern Stats stats;
void reset_stats();
void launch_impl(dim3 grid, dim3 block, bool has_barrier, const std::function<void()>& body);
void syncthreads();
template <class F> inline void launch(dim3 grid, dim3 block, bool has_barrier, F&& body) {
    launch_impl(grid, block, has_barrier, std::function<void()>(body));
}
template <class T> inline bool in_range(const textureReference& t, int i) {
    if (i >= 0 && t.ptr && ((size_t)i + 1) * sizeof(T) <= t.bytes) return true;
    stats.oob_fetches++;
    stats.last_oob++;
    return false;
}
}  // namespace cuda_host

template <class T>
static inline T tex1Dfetch(const texture<T, 1, cudaReadModeElementType>& t, int i) {
    T zero;
    memset(&zero, 0, sizeof(T));
    return cuda_host::in_range<T>(t, i) ? ((const T*)t.ptr)[i] : zero;
}
// Normalised read of unsigned 8-bit data: v / 255 in float.
static inline float tex1Dfetch(const texture<unsigned char, 1, cudaReadModeNormalizedFloat>& t,
                               int i) {
    if (!cuda_host::in_range<unsigned char>(t, i)) return 0.0f;
    return (float)((const unsigned char*)t.ptr)[i] / 255.0f;
}
// 2D fetch from pitched linear memory: unnormalised coordinates, point sampling (the texel
// that contains the coordinate, floor), clamped to the edge.  Other modes are not implemented.
template <class T>
static inline T tex2D(const texture<T, 2, cudaReadModeElementType>& t, float x, float y) {
    if (t.normalized || t.filterMode != cudaFilterModePoint || !t.ptr) abort();
    int ix = (int)floorf(x), iy = (int)floorf(y);
    const int cx = ix < 0 ? 0 : (ix > t.width - 1 ? t.width - 1 : ix);
    const int cy = iy < 0 ? 0 : (iy > t.height - 1 ? t.height - 1 : iy);
    if (cx != ix || cy != iy) {
        cuda_host::stats.clamped_2d++;
        cuda_host::stats.last_clamped++;
    }
    return *(const T*)((const char*)t.ptr + (size_t)cy * t.pitch + (size_t)cx * sizeof(T));
}

cudaError_t cudaMalloc(void** p, size_t bytes);
cudaError_t cudaFree(void* p);
static inline cudaError_t cudaFreeArray(cudaArray*) { return cudaSuccess; }
static inline cudaError_t cudaMemcpy(void* d, const void* s, size_t n, cudaMemcpyKind) {
    memcpy(d, s, n);
    return cudaSuccess;
}
static inline cudaError_t cudaMemcpyAsync(void* d, const void* s, size_t n, cudaMemcpyKind,
                                          cudaStream_t = 0) {
    memcpy(d, s, n);
    return cudaSuccess;
}
template <class T>
static inline cudaError_t cudaMemcpyToSymbol(T& symbol, const void* s, size_t n, size_t offset = 0,
                                             cudaMemcpyKind = cudaMemcpyHostToDevice) {
    memcpy((char*)&symbol + offset, s, n);
    return cudaSuccess;
}
static inline cudaError_t cudaBindTexture(size_t* offset, textureReference* t, const void* p,
                                          const cudaChannelFormatDesc*, size_t bytes) {
    if (offset) *offset = 0;
    t->ptr = p;
    t->bytes = bytes;
    t->width = t->height = 0;
    t->pitch = 0;
    return cudaSuccess;
}
static inline cudaError_t cudaBindTexture2D(size_t* offset, textureReference* t, const void* p,
                                            const cudaChannelFormatDesc*, size_t width,
                                            size_t height, size_t pitch) {
    if (offset) *offset = 0;
    t->ptr = p;
    t->bytes = pitch * height;
    t->width = (int)width;
    t->height = (int)height;
    t->pitch = pitch;
    return cudaSuccess;
}
static inline cudaError_t cudaThreadSynchronize() { return cudaSuccess; }
static inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
static inline cudaError_t cudaGetLastError() { return cudaSuccess; }
static inline const char* cudaGetErrorString(cudaError_t) { return "no error"; }
static inline cudaError_t cudaGetDeviceCount(int* n) { *n = 1; return cudaSuccess; }
static inline cudaError_t cudaGetDeviceProperties(cudaDeviceProp* p, int) {
    memset(p, 0, sizeof(*p));
    p->major = 1;
    return cudaSuccess;
}
static inline cudaError_t cudaSetDevice(int) { return cudaSuccess; }
static inline cudaError_t cudaGetDevice(int* d) { *d = 0; return cudaSuccess; }
// GL interop: nothing to map on the host.
static inline cudaError_t cudaGLRegisterBufferObject(unsigned) { return 1; }
static inline cudaError_t cudaGLUnregisterBufferObject(unsigned) { return 1; }
static inline cudaError_t cudaGLMapBufferObject(void** p, unsigned) { *p = nullptr; return 1; }
static inline cudaError_t cudaGLUnmapBufferObject(unsigned) { return 1; }
