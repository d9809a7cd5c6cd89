// timer_slots.h -- internal: the slot accounting of the per-class kernel timers (gnn_mlp_timing_*).  A timed launch takes the
// next slot of its class -- a (start, stop) event pair, created on first use and reused after every reset of `used` -- until
// the class is full.  Plain C++, no HIP: handle.h binds Event to hipEvent_t and `make` to hipEventCreate
// (tests/native/timer_slots_check.cpp binds them to its own).
#pragma once
#include <cstddef>
#include <vector>

namespace gnn {
namespace host {

constexpr size_t kTimerSlotsMax = 8192; // timed launches of one class between two resets; further ones run untimed

template <class Event> struct TimerSlots {
    std::vector<Event> start, stop; // the pairs created so far
    size_t used = 0;
    // make(Event *) -> bool creates one event.  false: the class is full or an event could not be created (nothing is taken)
    template <class Make> bool take(Make make, Event *e0, Event *e1) {
        if (used >= kTimerSlotsMax) return false;
        if (used >= start.size()) {
            Event a{}, b{};
            if (!make(&a) || !make(&b)) return false;
            start.push_back(a); stop.push_back(b);
        }
        *e0 = start[used]; *e1 = stop[used]; used++;
        return true;
    }
};

// the next slot of class `cls`; false (the launch runs untimed) when timing is off or the launch belongs to no class (cls < 0)
template <class Event, size_t N, class Make>
bool take_timer_slot(bool timing, TimerSlots<Event> (&classes)[N], int cls, Make make, Event *e0, Event *e1) {
    if (!timing || cls < 0 || cls >= (int)N) return false;
    return classes[cls].take(make, e0, e1);
}

} // namespace host
} // namespace gnn
