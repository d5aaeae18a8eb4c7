// A group of device buffers and events that exists completely or not at all. Plain C++, no HIP: the allocator calls are parameters,
// so the failure paths can be walked on the host (tests/all_or_nothing_check.cpp).
#pragma once

#include <cstddef>

namespace lw {

// Every slot is null on entry. alloc(void **, size_t) and create(Ev *) return true on success; release(void *) and destroy(Ev) undo them.
// On the first failure whatever was made is released again, every slot is null, and the result is false.
template <int NB, int NE, class Ev, class Alloc, class Release, class Create, class Destroy>
bool make_all_or_nothing(void **const (&bufs)[NB], const size_t (&bytes)[NB], Ev *const (&evs)[NE], Alloc alloc, Release release,
                         Create create, Destroy destroy)
{
    bool ok = true;
    for (int i = 0; i < NB && ok; ++i)
        if (!(ok = alloc(bufs[i], bytes[i]))) *bufs[i] = nullptr;
    for (int i = 0; i < NE && ok; ++i)
        if (!(ok = create(evs[i]))) *evs[i] = Ev{};
    if (ok) return true;
    for (int i = 0; i < NB; ++i)
        if (*bufs[i]) { release(*bufs[i]); *bufs[i] = nullptr; }
    for (int i = 0; i < NE; ++i)
        if (*evs[i]) { destroy(*evs[i]); *evs[i] = Ev{}; }
    return false;
}

}  // namespace lw
