/* ll_workspace.h -- host-side helpers of the objects that own device memory, once: a create-time allocation kept in the owner's list,
 * the carve of one grown buffer into typed parts, a table blob of 256-byte aligned parts, the time between two events.  How a buffer
 * GROWS stays with its owner: whether the old one is kept on failure, doubling, a floor and a wait before the free differ on purpose. */
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

static inline size_t ll_up256(size_t bytes) { return (bytes + 255) / 256 * 256; }

/* count elements (at least one) of device memory, freed with the owner's `allocs`; zero: cleared before the call returns.  false:
 * err says why, and what was allocated stays in allocs */
template <typename T>
static bool ll_dev_alloc(std::vector<void *> &allocs, std::string &err, T *&ptr, size_t count, bool zero)
{
    void *p = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    if (hipMalloc(&p, bytes) != hipSuccess) { err = "hipMalloc failed (" + std::to_string(bytes) + " bytes)"; return false; }
    allocs.push_back(p);
    if (zero && hipMemset(p, 0, bytes) != hipSuccess) { err = "hipMemset failed"; return false; }
    ptr = (T *)p;
    return true;
}

/* parts of one buffer, each rounded up to 256 bytes.  p == nullptr: size only -- the takes return nullptr and `at` ends at the need */
struct LLCarve {
    unsigned char *p; size_t at = 0;
    template <typename T> T *take(size_t count) { T *r = p ? (T *)(p + at) : nullptr; at += ll_up256(count * sizeof(T)); return r; }
};

/* a's elements appended to a table blob at the next multiple of 256 bytes; returns where they begin */
template <typename T>
static size_t ll_blob_put(std::vector<unsigned char> &blob, const std::vector<T> &a)
{
    const size_t at = ll_up256(blob.size());
    blob.resize(at + a.size() * sizeof(T));
    if (!a.empty()) std::memcpy(blob.data() + at, a.data(), a.size() * sizeof(T));
    return at;
}

/* milliseconds from event a to event b, both reached; fallback: what the caller reports when the query fails */
static inline double ll_event_ms(hipEvent_t a, hipEvent_t b, double fallback)
{
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : fallback;
}
