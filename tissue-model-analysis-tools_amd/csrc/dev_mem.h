// Owners of device and pinned memory in libtmat_hip.so.  Outside this header only constants allocate by hand (weights, gaussian /
// Lanczos / decision tables, the roi patch order), plus ws_get's slots (tmat_ctx.h) and the caller-owned blocks of tmat_dev_alloc.
//   WsList    what a handle or a pass geometry keeps: every block with its size, so that tmat_destroy, tmat_debug_poison and
//             tmat_debug_held_bytes walk ONE list
//   DevScope  what one call needs: released when the call returns, by whatever path
#pragma once
#include "tmat_internal.h"

#include <algorithm>
#include <map>
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

// Device allocations of one call, released together when it returns.  After a failed request `ok` is false and every later request
// returns null: take everything, then test `ok` once.
//   alloc   a plain hipMalloc, freed at scope end
//   pooled  a block of the handle's pool, which gets it back at scope end and hands it to the next call: a Z-stack call makes some
//           thirty allocations of a dozen sizes, and a hipMalloc / hipFree pair per block was a tenth of its time.  The pool only
//           ever holds what one call of each geometry needs; tmat_destroy frees it.
struct DevScope {
    WsPool &pool;
    std::vector<std::pair<void *, size_t>> blocks;      // the pool's
    std::vector<void *> owned;                          // alloc's
    bool ok = true;
    hipStream_t drain;                      // synchronised before anything is released: an early error return must not leave async work behind
    explicit DevScope(WsPool &p, hipStream_t drain_stream = nullptr) : pool(p), drain(drain_stream) {}
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
    ~DevScope()
    {
        if (drain) hipStreamSynchronize(drain);
        for (auto &b : blocks) pool.insert({b.second, b.first});
        for (void *p : owned) hipFree(p);
    }
};

}  // namespace tmat
