// hiprz_session.hpp — the host half that the libraries beside libhiprz.so share (query/hiprz_query.hip, order/hiprz_order.hip,
// bake/hiprz_bake.hip): a handle bound to a context, its error text, the context's device view, the pinned staging of host-pointer calls
// with its round trip, and what create, destroy and last_error do.  Host code on the HIP runtime, no __global__, and everything in an
// unnamed namespace: each library gets a copy of its own and exports nothing of it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "hiprz_device.hpp"

namespace hiprz {
namespace {

// host-pointer calls: pinned staging and its device twin, `capacity` records each
struct Staging {
    void *pinned_in = nullptr, *pinned_out = nullptr, *dev_in = nullptr, *dev_out = nullptr;
    size_t capacity = 0;

    void release() {
        if (dev_in) (void)hipFree(dev_in);  // (hipFree waits for whatever still uses the buffer)
        if (dev_out) (void)hipFree(dev_out);
        if (pinned_in) (void)hipHostFree(pinned_in);
        if (pinned_out) (void)hipHostFree(pinned_out);
        dev_in = dev_out = pinned_in = pinned_out = nullptr, capacity = 0;
    }

    // room for n records of in_bytes and out_bytes each (the largest record of either side), `capacity_rule(capacity, n)` of them; all four
    // allocations or none.  The device they are made on is the current one: call it after a view.
    hipError_t grow(size_t n, size_t in_bytes, size_t out_bytes, size_t (*capacity_rule)(size_t, size_t)) {
        if (n <= capacity) return hipSuccess;
        const size_t cap = capacity_rule(capacity, n);
        release();
        const auto pinned = [cap](void** p, size_t bytes) { return hipHostMalloc(p, cap * bytes, hipHostMallocDefault); };
        hipError_t e = hipMalloc(&dev_in, cap * in_bytes);
        if (e == hipSuccess) e = hipMalloc(&dev_out, cap * out_bytes);
        if (e == hipSuccess) e = pinned(&pinned_in, in_bytes);
        if (e == hipSuccess) e = pinned(&pinned_out, out_bytes);
        if (e == hipSuccess) capacity = cap;
        else release();
        return e;
    }
};

// what every handle is: struct hiprz_query, hiprz_order and hiprz_bake derive from it and add what is their own
struct Session {
    hiprz_ctx* ctx = nullptr;
    int device = -1;  // the context's head device, known from the first view on (hiprz_device_view makes it current)
    Staging staging;
    std::string error;
};

thread_local std::string g_error;  // of calls without a handle

int fail(Session* h, int code, const std::string& message) {
    (h ? h->error : g_error) = message;
    return code;
}
int fail_hip(Session* h, const char* what, hipError_t e) { return fail(h, HIPRZ_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

// the context's device views, fetched on every call; the sizes are the guard against a libhiprz.so built from other headers
int view(Session* h, const char* what, DScene& s, DCamera* cam = nullptr) {
    const int rc = hiprz_device_view(h->ctx, &s, sizeof s, cam, cam ? sizeof *cam : 0u);
    if (rc != HIPRZ_OK) {
        const char* why = hiprz_last_error(h->ctx);
        return fail(h, rc, std::string(what) + ": " + (why && *why ? why : "the context gave no device view"));
    }
    if (const hipError_t e = hipGetDevice(&h->device); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

hipStream_t stream_of(Session* h, void* stream) { return static_cast<hipStream_t>(stream ? stream : hiprz_stream(h->ctx)); }

int grow_staging(Session* h, const char* what, size_t n, size_t in_bytes, size_t out_bytes, size_t (*capacity_rule)(size_t, size_t)) {
    if (const hipError_t e = h->staging.grow(n, in_bytes, out_bytes, capacity_rule); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

// a host-pointer call once the staging holds n records: n records of in_bytes each go to the device on the context's stream,
// launch(dev_in, dev_out, stream) enqueues the work and returns HIPRZ_OK or what fail() gave it, n records of out_bytes each come back
template <typename Launch>
int round_trip(Session* h, const char* what, const void* in, size_t n, size_t in_bytes, void* out, size_t out_bytes, Launch launch) {
    const Staging& g = h->staging;
    hipStream_t st = stream_of(h, nullptr);
    std::memcpy(g.pinned_in, in, n * in_bytes);
    if (const hipError_t e = hipMemcpyAsync(g.dev_in, g.pinned_in, n * in_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const int rc = launch(g.dev_in, g.dev_out, st); rc != HIPRZ_OK) return rc;
    if (const hipError_t e = hipMemcpyAsync(g.pinned_out, g.dev_out, n * out_bytes, hipMemcpyDeviceToHost, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(h, what, e);
    std::memcpy(out, g.pinned_out, n * out_bytes);
    return HIPRZ_OK;
}

// the bodies of *_create, *_destroy and *_last_error; `name`: "query_create"
template <typename Handle>
int create(Handle** out, hiprz_ctx* ctx, const char* name) {
    if (!out) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(name) + ": null output");
    *out = nullptr;
    int n = 0;
    if (const hipError_t e = hipGetDeviceCount(&n); e != hipSuccess || n <= 0)
        return fail(nullptr, HIPRZ_ERR_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (!ctx) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(name) + ": null context");
    (*out = new Handle)->ctx = ctx;
    return HIPRZ_OK;
}

// owns_more: the handle holds device memory besides the staging, which release_more() frees; the handle's device is made current only when
// there is something to free on it
template <typename Handle, typename ReleaseMore>
int destroy(Handle* h, bool owns_more, ReleaseMore release_more) {
    if (!h) return HIPRZ_ERR_INVALID;
    if (h->staging.capacity || owns_more) {
        (void)hipSetDevice(h->device);
        h->staging.release();
        release_more();
    }
    delete h;
    return HIPRZ_OK;
}
template <typename Handle>
int destroy(Handle* h) { return destroy(h, false, [] {}); }

const char* last_error(const Session* h) { return h ? h->error.c_str() : g_error.c_str(); }

}  // namespace
}  // namespace hiprz
