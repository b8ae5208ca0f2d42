// Owners of device and pinned memory in libtmat_hip.so.  Outside this header only constants allocate by hand (weights, gaussian /
// Lanczos / decision tables, the roi patch order), plus ws_get's slots (tmat_ctx.h) and the caller-owned blocks of tmat_dev_alloc.
//   WsList    what a handle or a pass geometry keeps: every block with its size, so that tmat_destroy, tmat_debug_poison and
//             tmat_debug_held_bytes walk ONE list
//   DevScope  what one call needs, memory and the host <-> device copies around it: released when the call returns, by whatever path
// Lifetime rule: a host temporary that feeds or receives an asynchronous copy belongs to the scope (keep / host), which releases it
// only after it has drained its stream.
#pragma once
#include "../../include/tmat.h"
#include "tmat_internal.h"

#include <algorithm>
#include <map>
#include <memory>
#include <utility>

namespace tmat {

// a device / pinned workspace a forward or a pass writes before it reads (tmat_debug_poison fills exactly these)
struct WsEnt { void *p; size_t bytes; bool host; };

struct WsList {
    std::vector<WsEnt> ents;
    void *add(size_t bytes, bool host, const char *what)        // nullptr + set_error on failure
    {
        void *p = nullptr;
        const size_t nb = std::max<size_t>(bytes, 1);
        if (!hip_ok(host ? hipHostMalloc(&p, nb, hipHostMallocDefault) : hipMalloc(&p, nb), what)) return nullptr;
        ents.push_back(WsEnt{p, bytes, host});
        return p;
    }
    void *dev(size_t bytes, const char *what = "hipMalloc") { return add(bytes, false, what); }
    void *pinned(size_t bytes, const char *what = "hipHostMalloc") { return add(bytes, true, what); }
    static void free_ent(const WsEnt &e) { if (e.host) hipHostFree(e.p); else hipFree(e.p); }
    void release(void *p)       // one block back (a buffer that is re-made larger); null and foreign pointers are ignored
    {
        auto it = std::find_if(ents.begin(), ents.end(), [p](const WsEnt &e) { return e.p == p; });
        if (p && it != ents.end()) { free_ent(*it); ents.erase(it); }
    }
    void free_all() { for (const WsEnt &e : ents) free_ent(e); ents.clear(); }
    std::vector<WsEnt>::const_iterator begin() const { return ents.begin(); }
    std::vector<WsEnt>::const_iterator end() const { return ents.end(); }
};

using WsPool = std::multimap<size_t, void *>;       // released blocks by size (Ctx::ws_pool)

// Device allocations and transfers of one call on one stream, released together when it returns.  After a failed request `ok` is false
// and every later allocation, copy and finish does nothing and returns null / false: take everything, then test `ok` once; the error
// text stays the first failure's.  (check() only records the result of a call its caller has already made.)  A scope that carries
// copies needs its stream; nullptr is for the callers that only allocate and copy with blocking hipMemcpy: their h2d / d2h fail.
//   alloc   a plain hipMalloc, freed at scope end
//   pooled  a block of the handle's pool, which gets it back at scope end and hands it to the next call: a Z-stack call makes some
//           thirty allocations of a dozen sizes, and a hipMalloc / hipFree pair per block was a tenth of its time.  The pool only
//           ever holds what one call of each geometry needs; tmat_destroy frees it.
//   alloc_from / pooled_from   the same, filled from a host array (H2D on the stream)
//   h2d / d2h   copies on the stream, into and out of any device memory (ws_get slots, the handle's buffers); a null d2h target is skipped
//   keep / host a host temporary of such a copy (a table built inside the call, a flag or count read back): lives until the drain
//   finish      synchronise once -> TMAT_OK, or TMAT_E_HIP if anything in the scope failed; the destructor does not synchronise
//               again unless the scope has been used since
struct DevScope {
    WsPool &pool;
    std::vector<std::pair<void *, size_t>> blocks;      // the pool's
    std::vector<void *> owned;                          // alloc's
    std::vector<std::shared_ptr<void>> hosts;           // keep's: members go after the destructor's drain
    bool ok = true;
    bool drained = false;                   // finish() has synchronised and no operation of the scope has followed
    hipStream_t drain;                      // synchronised before anything is released: an early error return must not leave async work behind
    DevScope(WsPool &p, hipStream_t drain_stream) : pool(p), drain(drain_stream) {}
    DevScope(const DevScope &) = delete;
    DevScope &operator=(const DevScope &) = delete;
    template <typename T> T *alloc(size_t count, const char *what = "hipMalloc") { return (T *)alloc_bytes(count * sizeof(T), what); }
    void *alloc_bytes(size_t bytes, const char *what = "hipMalloc")
    {
        void *p = nullptr;
        if (!ok || !hip_ok(hipMalloc(&p, bytes), what)) { ok = false; return nullptr; }
        owned.push_back(p);
        return p;
    }
    template <typename T> T *pooled(size_t count) { return (T *)pooled_bytes(std::max<size_t>(count, 1) * sizeof(T)); }
    void *pooled_bytes(size_t bytes)
    {
        if (!ok) return nullptr;
        auto it = pool.lower_bound(bytes);
        if (it != pool.end() && it->first <= bytes + bytes / 4 + 4096) {          // close enough in size: reuse
            void *p = it->second;
            blocks.push_back({p, it->first});
            pool.erase(it);
            return p;
        }
        void *p = nullptr;
        if (!hip_ok(hipMalloc(&p, bytes), "hipMalloc")) { ok = false; return nullptr; }
        blocks.push_back({p, bytes});
        return p;
    }
    bool check(hipError_t e, const char *what)          // the result of any other call on the stream
    {
        drained = false;
        if (ok && !hip_ok(e, what)) ok = false;
        return ok;
    }
    bool streamed() { if (ok && !drain) { set_error("DevScope: a copy on a scope without a stream"); ok = false; } return ok; }
    bool h2d(void *dst, const void *src, size_t bytes) { return streamed() && check(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, drain), "H2D"); }
    bool d2h(void *dst, const void *src, size_t bytes) { return streamed() && (!dst || check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, drain), "D2H")); }
    template <typename T> T *alloc_from(const T *src, size_t count) { T *p = alloc<T>(count); return h2d(p, src, count * sizeof(T)) ? p : nullptr; }
    template <typename T> T *pooled_from(const T *src, size_t count) { T *p = pooled<T>(count); return h2d(p, src, count * sizeof(T)) ? p : nullptr; }
    template <typename T> T *keep(std::vector<T> &&v)
    {
        auto h = std::make_shared<std::vector<T>>(std::move(v));
        hosts.push_back(h);
        return h->data();
    }
    template <typename T> T *host(size_t count = 1) { return keep(std::vector<T>(count)); }       // zeroed
    int finish()
    {
        if (!streamed() || !check(hipStreamSynchronize(drain), "sync")) return TMAT_E_HIP;
        drained = true;
        return TMAT_OK;
    }
    ~DevScope()
    {
        if (drain && !drained) hipStreamSynchronize(drain);
        for (auto &b : blocks) pool.insert({b.second, b.first});
        for (void *p : owned) hipFree(p);
    }
};

}  // namespace tmat
