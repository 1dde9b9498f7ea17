// Host-side base of the opaque handles of include/fs2.h (fs2_engine, fs2_vocoder, fs2_sdp, fs2_mel, fs2_fd): the error message and
// its check macros, the store of expected / loaded weights, the owner of device allocations, the uploads, the workspace arena.
// Host only, header only.  A new handle derives its struct from ErrorBase, lists its tensors with WeightStore::expect in *_create,
// forwards *_load_weight to WeightStore::load, asks first_missing() at the top of *_finalize and uploads through DevAllocs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/fs2.h"
#include "fs2_common.h"
#include "fs2_kernels.h"

namespace fs2 {

// What *_last_error returns.  fail() writes the message and hands the status back, so `return h->fail(code, ...)` reads as one step.
struct ErrorBase {
    char err[512] = {0};
    int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, sizeof(err), fmt, ap);
        va_end(ap);
        return code;
    }
};

// HIP call or fail (h: pointer to a handle) / status or return
#define FS2_HIP(h, call)                                                                               \
    do {                                                                                               \
        hipError_t _s = (call);                                                                        \
        if (_s != hipSuccess) return (h)->fail(FS2_ERR_HIP, "%s: %s", #call, hipGetErrorString(_s));    \
    } while (0)
#define FS2_TRY(call)                  \
    do {                               \
        const int _r = (call);         \
        if (_r != FS2_OK) return _r;   \
    } while (0)

// The tensors a handle expects (reference state_dict names -> shape) and, between *_load_weight and *_finalize, their fp32 values.
struct WeightStore {
    struct Entry {
        std::vector<int64_t> shape;
        bool keep = true;  // false: shape-checked when loaded, its values dropped, not required at finalize (training-only tensors)
        bool loaded = false;
        std::vector<float> data;
    };
    std::map<std::string, Entry> t;

    void expect(const std::string& name, std::vector<int64_t> shape, bool keep = true) {
        Entry& e = t[name] = Entry();
        e.shape = std::move(shape);
        e.keep = keep;
    }
    bool empty() const { return t.empty(); }
    void clear() { t.clear(); }
    // name, data and shape not null; a name loaded twice is overwritten
    int load(ErrorBase& eb, const char* name, const float* data, const int64_t* shape, int ndim) {
        auto it = t.find(name);
        if (it == t.end()) return eb.fail(FS2_ERR_WEIGHT, "unknown weight name '%s'", name);
        Entry& e = it->second;
        bool same = (size_t)ndim == e.shape.size();
        size_t n = 1;
        for (int i = 0; same && i < ndim; ++i) {
            same = shape[i] == e.shape[i];
            n *= (size_t)e.shape[i];
        }
        if (!same) return eb.fail(FS2_ERR_WEIGHT, "shape mismatch for '%s'", name);
        e.loaded = true;
        if (e.keep) e.data.assign(data, data + n);
        return FS2_OK;
    }
    // the first expected tensor (in name order) that finalize needs and no load has brought; null when complete
    const char* first_missing() const {
        for (const auto& kv : t)
            if (kv.second.keep && !kv.second.loaded) return kv.first.c_str();
        return nullptr;
    }
    const Entry& at(const std::string& name) const { return t.at(name); }
    void drop() {  // the host copies, once they are packed
        for (auto& kv : t) std::vector<float>().swap(kv.second.data);
    }
};

// Device allocations that live as long as their owner.
struct DevAllocs {
    std::vector<void*> p;
    DevAllocs() = default;
    DevAllocs(const DevAllocs&) = delete;
    DevAllocs& operator=(const DevAllocs&) = delete;
    ~DevAllocs() { for (void* q : p) (void)hipFree(q); }
    hipError_t alloc(void** out, size_t bytes) {
        const hipError_t s = hipMalloc(out, bytes ? bytes : 256);
        if (s == hipSuccess) p.push_back(*out);
        return s;
    }
    void swap(DevAllocs& o) { p.swap(o.p); }
};

// `oom`: the status of a failed hipMalloc (the engine reports FS2_ERR_NOMEM, the other handles FS2_ERR_HIP)
inline int dev_alloc(ErrorBase& eb, DevAllocs& a, void** out, size_t bytes, int oom) {
    if (a.alloc(out, bytes) != hipSuccess) return eb.fail(oom, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(hipGetLastError()));
    return FS2_OK;
}
// host bytes -> a new allocation of `a`
inline int upload_bytes(ErrorBase& eb, DevAllocs& a, const void* h, size_t bytes, void** out, int oom) {
    FS2_TRY(dev_alloc(eb, a, out, bytes, oom));
    FS2_HIP(&eb, hipMemcpy(*out, h, bytes, hipMemcpyHostToDevice));
    return FS2_OK;
}
// n fp32 host values -> storage dtype dt on the device, rounded as a device store of that type rounds, bit for bit
inline int upload_as(ErrorBase& eb, DevAllocs& a, const float* h, size_t n, int dt, void** out, int oom) {
    if (dt == FS2_F32) return upload_bytes(eb, a, h, n * 4, out, oom);
    if (!is_16bit(dt)) return eb.fail(FS2_ERR_ARG, "upload_as: not a storage dtype");
    std::vector<unsigned short> tmp(n);
    if (dt == FS2_F16) for (size_t i = 0; i < n; ++i) tmp[i] = f32_to_f16_sat(h[i]).v;
    else for (size_t i = 0; i < n; ++i) tmp[i] = f32_to_bf16(h[i]).v;
    return upload_bytes(eb, a, tmp.data(), n * 2, out, oom);
}

// One device block of packed weights, laid out on the host first: grow() appends a zero-filled region and returns its byte offset.
struct WeightBlock {
    std::vector<unsigned char> host;
    size_t grow(size_t bytes, size_t align) {
        const size_t at = host.size();
        host.resize(at + (bytes + align - 1) / align * align);
        return at;
    }
    int upload(ErrorBase& eb, DevAllocs& a, void** out) { return upload_bytes(eb, a, host.data(), host.size(), out, FS2_ERR_HIP); }
};

struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0;
    bool external = false;  // caller-owned memory (fs2_set_workspace): never freed or grown here
    bool overflow = false;  // a take() since the last reserve() did not fit (a null result cannot say so: offset 0 of a counting arena is null)
    // An arena that only counts: no memory behind it, every take() fits and hands out no pointer; a layout function run on it leaves
    // the size of its region in `off`.
    static Arena counting() {
        Arena a;
        a.cap = ~(size_t)0;
        return a;
    }
    int reserve(size_t bytes) {
        off = 0;
        overflow = false;
        if (bytes <= cap) return FS2_OK;
        if (external) return FS2_ERR_NOMEM;
        if (base) (void)hipFree(base);
        base = nullptr;
        cap = 0;
        bytes += bytes / 8;  // slack so slowly growing shapes do not reallocate every call
        if (hipMalloc((void**)&base, bytes) != hipSuccess) return FS2_ERR_NOMEM;
        cap = bytes;
        return FS2_OK;
    }
    void* take(size_t bytes) {
        const size_t a = (off + 255) & ~(size_t)255;
        if (a + bytes > cap) { overflow = true; return nullptr; }
        off = a + bytes;
        return base ? base + a : nullptr;
    }
    void release() {
        if (base && !external) (void)hipFree(base);
        base = nullptr;
        cap = off = 0;
        external = false;
    }
    void adopt(void* p, size_t bytes) {  // p == nullptr: back to an engine-owned, grow-only arena
        release();
        if (p) { base = (char*)p; cap = bytes; external = true; }
    }
};
inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace fs2
