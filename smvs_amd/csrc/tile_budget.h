// Barrier kernels (the resident PCG: every workgroup of a launch must be
// co-resident, one per CU) share a device by a TILE BUDGET: a Newton loop
// (newton_loop.hip holds its share for the whole loop, patch kernels included) or a
// single solve acquires as many tiles as its grid has workgroups and waits
// while the tiles in use plus its own exceed the device's CUs.  A full-size
// solve (256 tiles at 1920x1080, scale 2) therefore still runs alone, but the
// loops of the coarse scales -- 1, 4, 16, 64 tiles -- of several views in
// flight run side by side instead of taking turns (round 3's exclusive lock).
// Requests are served in arrival order, so a large request is not starved by
// a stream of small ones.  Across PROCESSES that share the GPU the budget
// cannot be shared; there an advisory lock on a file named after the device's
// PCI bus id still makes the processes take turns: two such kernels of two
// processes started together could each hold half of the CUs and wait for the
// other half for ever.  The file lock is taken without the mutex held, kept
// while loops of this process follow each other, and handed back after 100 ms at
// the latest so that a process waiting for it gets its turn (tile_budget.cc).
//
// Plain POSIX, no HIP: what the device has to say (its CUs, its bus id) comes
// in through bind(), cg_resident_budget (cg_resident.hip) asks for it.
#pragma once

#include <chrono>
#include <condition_variable>
#include <mutex>

namespace smvs_hip {

class DeviceTileBudget {
public:
    // capacity in tiles and the key the lock file is named after: once, the
    // first call counts.  acquire() needs it done.
    void bind(int capacity, const char *key);
    bool is_bound(void);
    void acquire(int tiles);
    void release(int tiles);
private:
    bool take_file_lock(void);
    void unlock_file(void);
    std::mutex mutex;
    std::condition_variable turn;
    int capacity = 0, used = 0, holders = 0;
    unsigned long long next_ticket = 0, serving = 0;
    int fd = -1;
    bool bound = false, file_locked = false;
    std::chrono::steady_clock::time_point file_since{}, no_file_until{};
};

struct ScopedTileBudget {
    DeviceTileBudget &budget;
    int tiles;
    ScopedTileBudget(DeviceTileBudget &budget_, int tiles_) : budget(budget_), tiles(tiles_)
    {
        budget.acquire(tiles);
    }
    ~ScopedTileBudget() { budget.release(tiles); }
    ScopedTileBudget(ScopedTileBudget const &) = delete;
    ScopedTileBudget &operator=(ScopedTileBudget const &) = delete;
};

} // namespace smvs_hip
