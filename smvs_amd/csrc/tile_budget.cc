// The tile budget of the barrier kernels (tile_budget.h): plain POSIX, built by
// the host compiler.
#include "tile_budget.h"

#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

namespace smvs_hip {

void
DeviceTileBudget::bind(int capacity_, const char *key)
{
    std::lock_guard<std::mutex> guard(mutex);
    if (bound)
        return;
    bound = true;
    capacity = capacity_;
    std::string name(key);
    for (char &c : name)
        if (c == ':' || c == '/')
            c = '_';
    // SMVS_LOCK_DIR, else the user's runtime directory, else /tmp.  The file
    // is never followed through a symlink; when another user created it
    // (O_RDWR refused) a read-only descriptor serves flock() just as well.
    const char *dir = std::getenv("SMVS_LOCK_DIR");
    if (dir == nullptr || dir[0] == 0)
        dir = std::getenv("XDG_RUNTIME_DIR");
    if (dir == nullptr || dir[0] == 0)
        dir = "/tmp";
    std::string const path = std::string(dir) + "/smvs_hip_barrier_" + name + ".lock";
    fd = ::open(path.c_str(), O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0666);
    if (fd < 0)
        fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC | O_NOFOLLOW);
    if (fd < 0)
        std::fprintf(stderr, "[smvs_hip] no lock file %s (%s): the resident solver is "
            "serialised inside this process only; a second process on the same GPU may "
            "push it into the streaming kernels\n", path.c_str(), std::strerror(errno));
}

bool
DeviceTileBudget::is_bound(void)
{
    std::lock_guard<std::mutex> guard(mutex);
    return bound;
}

// The advisory file lock that makes PROCESSES sharing a GPU take turns with
// their barrier kernels.  Taken by the head of this process's line WITHOUT the
// budget's mutex held (it may sleep for as long as another process's loops
// run); kept while loops of this process follow each other, but for at most
// FILE_HOLD at a stretch: after that the next acquirer lets the loops in flight
// drain, returns the lock -- a process waiting on it gets its turn -- and takes
// it again (a drain every 100 ms costs the single process ~1 %).  A lock somebody holds for 20 s is not one of ours (or is stuck):
// go on without it for a while -- the worst case is a resident solve that times
// out into the streaming kernels, not a hang.
static constexpr auto FILE_HOLD = std::chrono::milliseconds(100);
static constexpr auto FILE_GIVE_UP = std::chrono::seconds(20);
static constexpr auto FILE_RETRY_AFTER = std::chrono::seconds(60);

bool
DeviceTileBudget::take_file_lock(void)
{
    // (no mutex held: the caller is the only thread of this process in here)
    auto const t0 = std::chrono::steady_clock::now();
    for (long spin = 0;; ++spin) {
        if (::flock(fd, LOCK_EX | LOCK_NB) == 0)
            return true;
        if (errno != EWOULDBLOCK && errno != EINTR)
            return false;
        if (std::chrono::steady_clock::now() - t0 > FILE_GIVE_UP) {
            static std::atomic<bool> warned{false};
            if (!warned.exchange(true))
                std::fprintf(stderr, "[smvs_hip] barrier lock file busy for 20 s: "
                    "continuing without it\n");
            return false;
        }
        if (spin < 64)
            std::this_thread::yield();
        else
            std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

void
DeviceTileBudget::unlock_file(void)
{
    if (fd >= 0 && file_locked)
        (void)::flock(fd, LOCK_UN);
    file_locked = false;
}

void
DeviceTileBudget::acquire(int tiles)
{
    std::unique_lock<std::mutex> guard(mutex);
    if (tiles > capacity)
        tiles = capacity;
    unsigned long long const ticket = next_ticket++;
    // in arrival order; the head of the line waits for its tiles, the others
    // wait for the head
    turn.wait(guard, [&] { return serving == ticket && used + tiles <= capacity; });
    auto const now = std::chrono::steady_clock::now();
    bool handed_back = false;
    if (fd >= 0 && now >= no_file_until) {
        if (file_locked && now - file_since > FILE_HOLD) {
            // this process has had the GPU's barrier kernels to itself long
            // enough: let its loops in flight end (nobody passes the head of the
            // line meanwhile) and hand the lock back before taking it again
            turn.wait(guard, [&] { return holders == 0; });
            unlock_file();
            handed_back = true;
        }
        if (!file_locked) {
            guard.unlock();
            // (flock is not FIFO and a waiting process polls every 50 us: taking
            // the lock again at once would win it back nearly every time, and
            // the waiter would starve into its 20 s give-up.  Four of its poll
            // periods are its turn.)
            if (handed_back)
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            bool const got = take_file_lock();
            guard.lock();
            file_locked = got;
            file_since = std::chrono::steady_clock::now();
            if (!got)
                no_file_until = file_since + FILE_RETRY_AFTER;
        }
    }
    used += tiles;
    serving += 1;
    holders += 1;
    guard.unlock();
    turn.notify_all();   // (the next in line may fit beside this one)
}

void
DeviceTileBudget::release(int tiles)
{
    {
        std::lock_guard<std::mutex> guard(mutex);
        if (tiles > capacity)
            tiles = capacity;
        used -= tiles;
        if (--holders == 0)
            unlock_file();      // (non-blocking)
    }
    turn.notify_all();
}

} // namespace smvs_hip
