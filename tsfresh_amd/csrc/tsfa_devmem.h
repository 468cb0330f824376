// Ownership of device memory in the host layer (tsfa_api.cpp, tsfa_relevance.hip, tsfa_pack_device.hip and the three small
// packers tsfa_pack_dense.hip, tsfa_pack_valid.hip, tsfa_pack_times.hip), the one family of error macros these files check
// their HIP calls with, and the one device check of their entry points (tsfa_check_device).  Host-only; needs nothing but
// the HIP runtime.
//
// Whoever allocates device memory holds it in a DevPtr or a DevBuf, as a local variable or as a member of an object on the
// heap, and the destructor frees it: a function returns from wherever it fails, and a new member of a plan, a pack or a
// window set needs no line in a destroy function.  Memory that leaves through the C-ABI (tsfa_device_alloc) or that
// several holders share (pk_share) is handed off with release().
//
// RULE: no owner at namespace or static scope (thread_local included).  Its destructor would run at exit, after the HIP
// runtime may have unloaded, and hipFree on an unloaded runtime crashes.  Owners live on the stack or inside objects that
// a destroy function of the C-ABI deletes.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/tsfresh_amd.h"

int tsfa_fail(int code, const char *msg);  // tsfa_api.cpp: records the thread-local message, returns code

// Move-only owner of one hipMalloc allocation.  It frees on the device that is current when it goes: objects that outlive
// a call set their device first (~tsfa_plan, tsfa_windows_destroy).
template <class T>
class DevPtr {
    T *p_ = nullptr;

  public:
    DevPtr() = default;
    DevPtr(DevPtr &&o) noexcept : p_(o.release()) {}
    DevPtr &operator=(DevPtr &&o) noexcept {
        if (this != &o) { reset(); p_ = o.release(); }
        return *this;
    }
    DevPtr(const DevPtr &) = delete;
    DevPtr &operator=(const DevPtr &) = delete;
    ~DevPtr() { reset(); }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    T *release() { T *q = p_; p_ = nullptr; return q; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    // frees what it held, then one hipMalloc of `bytes`; the caller words the message (HIP_TRY_MALLOC, HIP_TRY_ALLOC below)
    hipError_t alloc(size_t bytes) {
        reset();
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes);
        if (e == hipSuccess) p_ = (T *)q;
        return e;
    }
};

// Grow-only scratch buffer of a plan
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        // the larger buffer first: a failed request leaves the old one (and its contents' owner) intact, and the
        // out-of-memory error is taken off the thread -- callers with a fallback (chirp-z scratch -> Goertzel sweep) go on
        // to launch kernels, whose launch check reads hipGetLastError (round-5 ADVICE)
        size_t want = bytes + bytes / 8 + 4096;
        void *q = nullptr;
        if (hipMalloc(&q, want) != hipSuccess) {
            (void)hipGetLastError();
            if (p) { (void)hipFree(p); p = nullptr; cap = 0; }   // second try with the old buffer's bytes returned
            if (hipMalloc(&q, want) != hipSuccess) {
                (void)hipGetLastError();
                return -1;
            }
        }
        if (p) (void)hipFree(p);
        p = q;
        cap = want;
        return 0;
    }
};

// "<who>: <what>: <HIP's text>", or "<what>: <HIP's text>" where who is empty
inline int tsfa_fail_hip(const char *who, const std::string &what, hipError_t e) {
    return tsfa_fail(TSFA_ERR_HIP, ((*who ? std::string(who) + ": " : std::string()) + what + ": " + hipGetErrorString(e)).c_str());
}

// "<who>: no HIP device visible: tsfresh_amd has no CPU fallback" on a box without a device, "<who>: no such HIP device" for
// an ordinal it does not have.  With a note (tsfa_relevance.hip; it may be empty) both cases read
// "<who>: no such HIP device<note>".
inline int tsfa_check_device(const char *who, int32_t device, const char *note = nullptr) {
    int ndev = 0;
    const bool none = hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1;
    if (none && !note) return tsfa_fail(TSFA_ERR_NO_DEVICE, (std::string(who) + ": no HIP device visible: tsfresh_amd has no CPU fallback").c_str());
    if (none || device < 0 || device >= ndev)
        return tsfa_fail(TSFA_ERR_NO_DEVICE, (std::string(who) + ": no such HIP device" + (note ? note : "")).c_str());
    return TSFA_OK;
}

// The function the messages name: a string literal, redefined in front of each entry point that wants its name in them
// (the packer files), or `who` in front of helpers that several entry points share and that take the name as an argument
// or hold it as a member (tsfa_pack_device.hip); empty elsewhere.
#ifndef TSFA_WHO
#define TSFA_WHO ""
#endif

// Each macro records the failure of a HIP call as the thread's last error and RETURNS TSFA_ERR_HIP from the function it
// stands in: with every allocation in an owner there is nothing to jump to.
#define HIP_TRY(expr)                                                    \
    do {                                                                 \
        const hipError_t e_ = (expr);                                    \
        if (e_ != hipSuccess) return tsfa_fail_hip(TSFA_WHO, #expr, e_); \
    } while (0)

// hipMalloc into an owner; the message shows the call as hipMalloc((void **)&owner, bytes)
#define HIP_TRY_MALLOC(owner, bytes)                                                                             \
    do {                                                                                                         \
        const hipError_t e_ = (owner).alloc(bytes);                                                              \
        if (e_ != hipSuccess) return tsfa_fail_hip(TSFA_WHO, "hipMalloc((void **)&" #owner ", " #bytes ")", e_); \
    } while (0)

// hipMalloc into an owner (one byte where none is asked for); the message names the byte count and what it was for
#define HIP_TRY_ALLOC(owner, bytes, what)                                                                                           \
    do {                                                                                                                            \
        const size_t nb_ = (size_t)(bytes);                                                                                         \
        const hipError_t e_ = (owner).alloc(nb_ ? nb_ : 1);                                                                         \
        if (e_ != hipSuccess)                                                                                                       \
            return tsfa_fail_hip(TSFA_WHO, "cannot allocate " + std::to_string(nb_) + " bytes of device memory for " + (what), e_); \
    } while (0)
