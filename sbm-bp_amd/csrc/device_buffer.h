// The one owner of device and page-locked host memory. Plain C++14: the buffer is a template over an
// allocator policy, so it compiles without HIP (tests/sanitize/buffer_sanitize.cpp runs it over a counting fake); the two HIP
// policies at the end exist under hipcc only. Every d_* / h_* buffer of the engine, the replica batch, the multi-GPU driver
// and the communicator is declared as one of these types, and memory is allocated and freed nowhere else.
//
// A buffer does five things and converts to T *:
//   own      alloc(count) allocates max(count, 1) * sizeof(T) bytes (whatever it held is released first); the destructor frees
//   account  given a uint64_t * (the engine's device_bytes) it adds what it allocates and subtracts exactly that when it frees
//   grow     ensure(count): nothing when the capacity suffices, else free, then allocate (contents are not kept); a failure
//            leaves the buffer empty with capacity 0
//   replace  replace(count): the new memory is allocated first, a failure leaves the old in place; then it is move-assigned
//            over the old, which frees the old and settles the account
//   borrow   borrow(p): a view of somebody else's memory, never freed and never accounted (an owned buffer it is called on is
//            released first)
#ifndef SBMBP_DEVICE_BUFFER_H
#define SBMBP_DEVICE_BUFFER_H

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/sbmbp.h"
#include "host_graph.h"

namespace sbmbp {

// what a policy's allocate() answers: SBMBP_OK, or the error code of the failure and the runtime's words for it
struct alloc_status {
    int code;
    const char *text;
};

// Policy: static alloc_status allocate(void **p, size_t bytes); static void release(void *p); static const char *name().
template <typename T, typename Alloc>
class buffer {
public:
    buffer() = default;
    buffer(const buffer &) = delete;
    buffer &operator=(const buffer &) = delete;
    buffer(buffer &&o) noexcept { take(o); }
    buffer &operator=(buffer &&o) noexcept {
        if (this != &o) { reset(); take(o); }
        return *this;
    }
    ~buffer() { reset(); }

    int alloc(size_t count, uint64_t *account = nullptr) {
        reset();
        const size_t bytes = (count > 1 ? count : 1) * sizeof(T);
        void *p = nullptr;
        const alloc_status s = Alloc::allocate(&p, bytes);
        if (s.code != SBMBP_OK) {
            set_error(std::string(Alloc::name()) + "(" + std::to_string(bytes) + " B): " + s.text);
            return s.code;
        }
        p_ = static_cast<T *>(p);
        cap_ = count;
        bytes_ = bytes;
        acct_ = account;
        if (acct_) *acct_ += bytes_;
        return SBMBP_OK;
    }
    int ensure(size_t count, uint64_t *account = nullptr) { return count <= cap_ ? SBMBP_OK : alloc(count, account); }
    int replace(size_t count, uint64_t *account = nullptr) {
        buffer fresh;
        const int r = fresh.alloc(count, account);
        if (r != SBMBP_OK) return r;
        *this = static_cast<buffer &&>(fresh);
        return SBMBP_OK;
    }
    void borrow(T *p) {
        reset();
        p_ = p;
    }
    void reset() {
        if (bytes_) {
            Alloc::release(p_);
            if (acct_) *acct_ -= bytes_;
        }
        p_ = nullptr;
        cap_ = bytes_ = 0;
        acct_ = nullptr;
    }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }  // elements asked for; 0 when empty or borrowed
    bool owns() const { return bytes_ != 0; }

private:
    void take(buffer &o) {
        p_ = o.p_; cap_ = o.cap_; bytes_ = o.bytes_; acct_ = o.acct_;
        o.p_ = nullptr; o.cap_ = o.bytes_ = 0; o.acct_ = nullptr;
    }
    T *p_ = nullptr;
    size_t cap_ = 0, bytes_ = 0;  // bytes_ != 0: the memory is this object's, and bytes_ is what the account was charged
    uint64_t *acct_ = nullptr;
};

}  // namespace sbmbp

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace sbmbp {

struct hip_device_memory {
    static alloc_status allocate(void **p, size_t bytes) {
        const hipError_t r = hipMalloc(p, bytes);
        return alloc_status{r == hipSuccess ? SBMBP_OK : (r == hipErrorOutOfMemory ? SBMBP_ERR_NOMEM : SBMBP_ERR_HIP), hipGetErrorString(r)};
    }
    static void release(void *p) { (void)hipFree(p); }
    static const char *name() { return "hipMalloc"; }
};
struct hip_pinned_memory {  // (a page-locked allocation that fails is a runtime error, as it always was here)
    static alloc_status allocate(void **p, size_t bytes) {
        const hipError_t r = hipHostMalloc(p, bytes, hipHostMallocDefault);
        return alloc_status{r == hipSuccess ? SBMBP_OK : SBMBP_ERR_HIP, hipGetErrorString(r)};
    }
    static void release(void *p) { (void)hipHostFree(p); }
    static const char *name() { return "hipHostMalloc"; }
};
template <typename T> using device_buffer = buffer<T, hip_device_memory>;
template <typename T> using pinned_buffer = buffer<T, hip_pinned_memory>;

}  // namespace sbmbp
#endif  // __HIPCC__

#endif  // SBMBP_DEVICE_BUFFER_H
