/* fa_hip.hip -- the HIP runtime wrappers of fa_hip.h: device count, allocations, copies, events, streams, peers */
#include "common.hpp"

static int g_dev_count = -1;

extern "C" int fa_hip_device_count(void) {
    if (g_dev_count < 0) {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess) { n = 0; (void)hipGetLastError(); }
        g_dev_count = n;
    }
    return g_dev_count;
}

/* NULL when the device cannot provide the memory (the planners then return NULL, like the reference's
   planner does when a solver's buffers cannot be had); every other HIP error is fatal */
extern "C" void *fa_hip_malloc(size_t nbytes) {
    void *p = NULL;
    if (nbytes == 0) nbytes = 16;
    hipError_t e = hipMalloc(&p, nbytes);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
        (void)hipGetLastError();
        fprintf(stderr, "fftw3_amd: the device cannot allocate %zu bytes\n", nbytes);
        return NULL;
    }
    FA_CHECK(e);
    return p;
}

extern "C" void fa_hip_free(void *p) {
    if (p) FA_CHECK(hipFree(p));
}

extern "C" void *fa_hip_host_malloc(size_t nbytes) {
    if (fa_hip_device_count() <= 0) return NULL;
    void *p = NULL;
    if (hipHostMalloc(&p, nbytes ? nbytes : 16, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return NULL;
    }
    return p;
}

extern "C" int fa_hip_host_free(void *p) {
    if (fa_hip_device_count() <= 0) return 0;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (attr.type == hipMemoryTypeHost) { FA_CHECK(hipHostFree(p)); return 1; }
    return 0;
}

extern "C" int fa_hip_is_device_ptr(const void *p) {
    if (!p || fa_hip_device_count() <= 0) return 0;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

/* ordinal of the device that owns a device allocation, -1 for anything else */
extern "C" int fa_hip_ptr_device(const void *p) {
    if (!p || fa_hip_device_count() <= 0) return -1;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
    if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged) return -1;
    return attr.device;
}

extern "C" void fa_hip_memcpy_h2d(void *dst, const void *src, size_t n, void *stream) {
    FA_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, (hipStream_t)stream));
}
extern "C" void fa_hip_memcpy_d2h(void *dst, const void *src, size_t n, void *stream) {
    FA_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, (hipStream_t)stream));
}
extern "C" void fa_hip_memset(void *dst, int v, size_t n, void *stream) {
    FA_CHECK(hipMemsetAsync(dst, v, n, (hipStream_t)stream));
}
extern "C" void fa_hip_stream_sync(void *stream) {
    FA_CHECK(hipStreamSynchronize((hipStream_t)stream));
}

extern "C" void *fa_hip_event_create(void) {
    hipEvent_t e;
    FA_CHECK(hipEventCreate(&e));
    return (void *)e;
}
extern "C" void fa_hip_event_record(void *ev, void *stream) {
    FA_CHECK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
}
extern "C" float fa_hip_event_elapsed_ms(void *a, void *b) {
    float ms = 0.f;
    FA_CHECK(hipEventElapsedTime(&ms, (hipEvent_t)a, (hipEvent_t)b));
    return ms;
}
extern "C" void fa_hip_event_destroy(void *ev) { FA_CHECK(hipEventDestroy((hipEvent_t)ev)); }
extern "C" void *fa_hip_stream_create(void) {
    hipStream_t s;
    FA_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    return (void *)s;
}
extern "C" void fa_hip_stream_destroy(void *s) { FA_CHECK(hipStreamDestroy((hipStream_t)s)); }
extern "C" int fa_hip_get_device(void) { int d = 0; FA_CHECK(hipGetDevice(&d)); return d; }
extern "C" void fa_hip_set_device(int dev) { FA_CHECK(hipSetDevice(dev)); }
/* 0 when dev may address peer's memory, 1 when there is no peer path.  The batch-sharding layer ignores a missing
   path (hipMemcpyPeerAsync stages through the host then); the slab planners return NULL for it, because their
   exchanges read the peer's memory directly */
extern "C" int fa_hip_enable_peer(int dev, int peer) {
    int can = 0, cur = 0;
    if (dev == peer) return 0;
    FA_CHECK(hipGetDevice(&cur));
    if (hipDeviceCanAccessPeer(&can, dev, peer) != hipSuccess || !can) { (void)hipGetLastError(); return 1; }
    FA_CHECK(hipSetDevice(dev));
    hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
    if (e != hipSuccess) (void)hipGetLastError();            /* hipErrorPeerAccessAlreadyEnabled included */
    FA_CHECK(hipSetDevice(cur));
    return (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) ? 0 : 1;
}
extern "C" void fa_hip_memcpy_peer(void *dst, int dst_dev, const void *src, int src_dev, size_t n, void *stream) {
    if (dst_dev == src_dev) FA_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    else FA_CHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, n, (hipStream_t)stream));
}
extern "C" void fa_hip_memcpy2d_peer(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, void *stream) {
    if (!width || !height) return;
    FA_CHECK(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToDevice, (hipStream_t)stream));
}
extern "C" void fa_hip_stream_wait_event(void *s, void *ev) {
    FA_CHECK(hipStreamWaitEvent((hipStream_t)s, (hipEvent_t)ev, 0));
}
