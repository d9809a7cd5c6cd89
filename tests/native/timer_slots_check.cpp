// Stand-alone host check of csrc/timer_slots.h (no HIP, no GPU): the slot accounting behind ScopedTimer, launch_timed and
// launch_instance (csrc/handle.h).  Events are ints handed out by a counting maker that can be told to fail.
// Built and run by tests/test_timer_slots_cpu.py, with -fsanitize=address,undefined and plainly.
#include "../../graph-neural-net_amd/csrc/timer_slots.h"

#include <cstdio>
#include <cstdlib>

using gnn::host::kTimerSlotsMax;
using gnn::host::take_timer_slot;
using gnn::host::TimerSlots;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

struct Maker { // event n is the int n (1, 2, ...); fails from the `fail_from`-th creation on
    int made = 0, fail_from = -1;
    bool operator()(int *e) { if (fail_from >= 0 && made + 1 >= fail_from) return false; *e = ++made; return true; }
};

int main() {
    Maker mk;
    auto make = [&](int *e) { return mk(e); };
    TimerSlots<int> cls[5];
    int a = -1, b = -1;

    // no slot: timing off, a launch of no class, a class that does not exist -- nothing created, nothing counted
    CHECK(!take_timer_slot(false, cls, 0, make, &a, &b));
    CHECK(!take_timer_slot(true, cls, -1, make, &a, &b));
    CHECK(!take_timer_slot(true, cls, 5, make, &a, &b));
    CHECK(mk.made == 0 && a == -1 && b == -1);
    for (const auto &c : cls) CHECK(c.used == 0 && c.start.empty() && c.stop.empty());

    // a pair per slot, created on first use, per class
    CHECK(take_timer_slot(true, cls, 2, make, &a, &b) && a == 1 && b == 2);
    CHECK(take_timer_slot(true, cls, 2, make, &a, &b) && a == 3 && b == 4);
    CHECK(take_timer_slot(true, cls, 4, make, &a, &b) && a == 5 && b == 6);
    CHECK(cls[2].used == 2 && cls[4].used == 1 && cls[0].used == 0 && mk.made == 6);

    // after a reset (gnn_mlp_timing_enable sets used = 0) the created pairs are handed out again, in order, before any new one
    cls[2].used = 0;
    CHECK(take_timer_slot(true, cls, 2, make, &a, &b) && a == 1 && b == 2);
    CHECK(take_timer_slot(true, cls, 2, make, &a, &b) && a == 3 && b == 4);
    CHECK(mk.made == 6);
    CHECK(take_timer_slot(true, cls, 2, make, &a, &b) && a == 7 && b == 8 && mk.made == 8);

    // the cap: kTimerSlotsMax slots, then the class is full (other classes are not)
    TimerSlots<int> &c0 = cls[0];
    for (size_t i = 0; i < kTimerSlotsMax; i++) CHECK(c0.take(make, &a, &b));
    CHECK(c0.used == kTimerSlotsMax && c0.start.size() == kTimerSlotsMax && c0.stop.size() == kTimerSlotsMax);
    const int made_at_cap = mk.made;
    a = b = -1;
    CHECK(!c0.take(make, &a, &b) && !take_timer_slot(true, cls, 0, make, &a, &b));
    CHECK(c0.used == kTimerSlotsMax && mk.made == made_at_cap && a == -1 && b == -1);
    CHECK(take_timer_slot(true, cls, 1, make, &a, &b));
    c0.used = 0; // ... and a full class is whole again after a reset, without a new event
    const int made_before = mk.made;
    for (size_t i = 0; i < kTimerSlotsMax; i++) CHECK(c0.take(make, &a, &b));
    CHECK(mk.made == made_before && !c0.take(make, &a, &b));

    // an event that cannot be created: no slot, the class unchanged; the second of a pair failing as well
    TimerSlots<int> &c3 = cls[3];
    mk.fail_from = mk.made + 1;
    a = b = -1;
    CHECK(!c3.take(make, &a, &b) && c3.used == 0 && c3.start.empty() && c3.stop.empty() && a == -1 && b == -1);
    mk.fail_from = mk.made + 2;
    CHECK(!c3.take(make, &a, &b) && c3.used == 0 && c3.start.empty() && c3.stop.empty() && a == -1 && b == -1);
    mk.fail_from = -1;
    CHECK(c3.take(make, &a, &b) && c3.used == 1 && c3.start.size() == 1 && c3.stop.size() == 1 && c3.start[0] == a && c3.stop[0] == b);

    std::printf("timer slots ok\n");
    return 0;
}
