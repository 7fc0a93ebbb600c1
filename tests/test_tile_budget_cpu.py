"""The tile budget of the barrier kernels (smvs_amd/csrc/tile_budget.cc) on the
CPU: plain POSIX code, built here with g++ behind a small extern "C" shim.
What is asserted is what acquire / release do, read off the code:
tiles > capacity is CLAMPED to the capacity (in both), requests are served in
arrival order, processes take turns through flock() on a file in SMVS_LOCK_DIR,
and without that file the budget still accounts inside the process."""
import ctypes as C
import fcntl
import os
import subprocess
import sys
import threading
import time

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smvs_amd", "csrc")
HOLD = 0.02     # seconds a holder keeps its tiles

SHIM = r"""
#include "tile_budget.h"
using smvs_hip::DeviceTileBudget;
extern "C" {
void *tb_new(int capacity, const char *key)
{
    DeviceTileBudget *b = new DeviceTileBudget;
    b->bind(capacity, key);
    return b;
}
void tb_acquire(void *b, int tiles) { static_cast<DeviceTileBudget *>(b)->acquire(tiles); }
void tb_release(void *b, int tiles) { static_cast<DeviceTileBudget *>(b)->release(tiles); }
void tb_delete(void *b) { delete static_cast<DeviceTileBudget *>(b); }
}
"""


def load(path):
    lib = C.CDLL(path)
    lib.tb_new.restype = C.c_void_p
    lib.tb_new.argtypes = [C.c_int, C.c_char_p]
    for f in (lib.tb_acquire, lib.tb_release):
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_int]
    lib.tb_delete.restype = None
    lib.tb_delete.argtypes = [C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def so_path(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_budget")
    shim = d / "shim.cc"
    shim.write_text(SHIM)
    out = str(d / "libtile_budget_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-Wall", "-Werror", "-fPIC", "-shared",
                           "-I", CSRC, "-o", out, os.path.join(CSRC, "tile_budget.cc"), str(shim)])
    return out


@pytest.fixture
def lock_dir(tmp_path, monkeypatch):
    monkeypatch.setenv("SMVS_LOCK_DIR", str(tmp_path))
    return tmp_path


def returns(fn, seconds=30.0):
    """fn() in a thread of its own -> did it come back?  (a wait that never ends
    fails the test instead of hanging it)"""
    t = threading.Thread(target=fn, daemon=True)
    t.start()
    t.join(seconds)
    return not t.is_alive()


def waits_for_release(lib, b, held, wanted):
    """With `held` tiles acquired, does a request for `wanted` come in only
    after they are released?"""
    assert returns(lambda: lib.tb_acquire(b, held))
    events = []

    def second():
        lib.tb_acquire(b, wanted)
        events.append("in")
        lib.tb_release(b, wanted)

    t = threading.Thread(target=second, daemon=True)
    t.start()
    time.sleep(HOLD)
    events.append("released")
    lib.tb_release(b, held)
    t.join(30.0)
    assert not t.is_alive()
    return events == ["released", "in"]


def two_threads(lib, b):
    """3 + 3 tiles of a capacity of 4 -> the most that were held at one time"""
    state = {"held": 0, "most": 0, "served": 0}
    guard = threading.Lock()
    start = threading.Barrier(2)

    def holder():
        start.wait()
        lib.tb_acquire(b, 3)
        with guard:
            state["held"] += 3
            state["most"] = max(state["most"], state["held"])
        time.sleep(HOLD)
        with guard:
            state["held"] -= 3
            state["served"] += 1
        lib.tb_release(b, 3)

    threads = [threading.Thread(target=holder, daemon=True) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30.0)
    assert not any(t.is_alive() for t in threads)
    assert state["served"] == 2 and state["held"] == 0
    return state["most"]


def test_request_above_capacity_is_clamped(so_path, lock_dir):
    lib = load(so_path)
    b = lib.tb_new(4, b"0000:clamp:00.0")
    # acquire: 10 of 4 tiles is served as 4 (it returns, and the budget is full)
    assert waits_for_release(lib, b, 10, 1)
    # release clamps the same way: the 4 tiles are back, no more and no fewer
    assert waits_for_release(lib, b, 4, 4)
    assert waits_for_release(lib, b, 3, 2)
    lib.tb_delete(b)
    # the key's ':' and '/' do not reach the file name
    assert os.listdir(lock_dir) == ["smvs_hip_barrier_0000_clamp_00.0.lock"]


def test_two_threads_take_turns(so_path, lock_dir):
    lib = load(so_path)
    b = lib.tb_new(4, b"threads")
    assert two_threads(lib, b) == 3
    lib.tb_delete(b)


# One process of the two-process test: ROUNDS times 3 tiles of 4, counted in a
# file "<held> <most held> <times served>" that the holders update under a lock
# of its own.
WORKER = r"""
import fcntl, sys, time
sys.path.insert(0, sys.argv[1])
import test_tile_budget_cpu as T
print("ready", flush=True)
sys.stdin.readline()
T.hold_rounds(T.load(sys.argv[2]), sys.argv[3], int(sys.argv[4]))
"""


def count(counter, delta):
    with open(counter, "r+") as f:
        fcntl.flock(f, fcntl.LOCK_EX)
        held, most, served = (int(v) for v in f.read().split())
        held += delta
        f.seek(0)
        f.truncate()
        f.write("%d %d %d" % (held, max(most, held), served + (1 if delta > 0 else 0)))


def hold_rounds(lib, counter, rounds):
    b = lib.tb_new(4, b"processes")
    for _ in range(rounds):
        lib.tb_acquire(b, 3)
        count(counter, 3)
        time.sleep(HOLD)
        count(counter, -3)
        lib.tb_release(b, 3)
    lib.tb_delete(b)


def test_two_processes_share_the_lock_file(so_path, lock_dir):
    rounds = 8
    counter = str(lock_dir / "counter")
    with open(counter, "w") as f:
        f.write("0 0 0")
    child = subprocess.Popen([sys.executable, "-c", WORKER, os.path.dirname(os.path.abspath(__file__)),
                              so_path, counter, str(rounds)],
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert child.stdout.readline().strip() == "ready"
        child.stdin.write("go\n")
        child.stdin.flush()
        assert returns(lambda: hold_rounds(load(so_path), counter, rounds), 120.0)
        assert child.wait(120.0) == 0
    finally:
        if child.poll() is None:
            child.kill()
            child.wait()
    held, most, served = (int(v) for v in open(counter).read().split())
    assert held == 0 and served == 2 * rounds
    assert most <= 4      # (3: never both)


@pytest.mark.parametrize("kind", ["read_only", "not_a_directory"])
def test_without_a_lock_file_the_process_accounts_alone(so_path, tmp_path, monkeypatch, capfd, kind):
    if kind == "read_only":
        lock_dir = tmp_path / "ro"
        lock_dir.mkdir()
        lock_dir.chmod(0o555)
    else:
        lock_dir = tmp_path / "file"
        lock_dir.write_text("")
    monkeypatch.setenv("SMVS_LOCK_DIR", str(lock_dir))
    lib = load(so_path)
    b = lib.tb_new(4, b"fallback")
    try:
        # (a read-only directory does not stop the superuser: there the file exists)
        if not os.access(str(lock_dir), os.W_OK):
            assert "no lock file" in capfd.readouterr().err
            assert not lock_dir.is_dir() or os.listdir(lock_dir) == []
        assert two_threads(lib, b) == 3
        assert waits_for_release(lib, b, 10, 1)
    finally:
        lib.tb_delete(b)
        if kind == "read_only":
            lock_dir.chmod(0o755)
