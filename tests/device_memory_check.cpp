// Host check of the owning types of open_ludwig_amd/csrc/device_memory.hpp and of the idiom the step library uses them in: make locals,
// move them into the members once every call has succeeded. The runtime is a counting stand-in that fails at a chosen call.
// tests/test_library_abi.py builds it with -fsanitize=address,undefined, so leaks, double frees and uses of released memory are reported too.
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "device_memory.hpp"

namespace {

struct Event { int id; };

int g_calls = 0, g_fail_at = -1, g_live = 0, g_released = 0;

struct FakeMem {
    static int alloc(void **p, size_t n)
    {
        if (g_calls++ == g_fail_at) { *p = reinterpret_cast<void *>(0x1); return 2; }     // a failed call may leave rubbish behind
        *p = malloc(n);
        ++g_live;
        return 0;
    }
    static void release(void *p) { free(p); --g_live; ++g_released; }
};
struct FakeEventOps {
    static int create(Event **e)
    {
        if (g_calls++ == g_fail_at) return 2;
        *e = new Event{g_calls};
        ++g_live;
        return 0;
    }
    static int destroy(Event *e) { delete e; --g_live; ++g_released; return 0; }
};
template <class T> using Dev = lw::DeviceArray<T, FakeMem>;
using Ev = lw::DeviceHandle<Event *, FakeEventOps>;

// the second set of interface side buffers, as make_second_iface_set makes it: four arrays and two events, all of them or none
struct Set {
    Dev<float> side, side2;
    Dev<double> mac, mac2;
    Ev done[2];
    long counted = 0;
};

bool make_set(Set &s)
{
    Dev<float> side, side2;
    Dev<double> mac, mac2;
    Ev done[2];
    int e = side.alloc(16);
    if (!e) e = side2.alloc(16);
    if (!e) e = mac.alloc(2);
    if (!e) e = mac2.alloc(2);
    if (!e) e = done[0].create();
    if (!e) e = done[1].create();
    if (e) return false;
    s.side = std::move(side); s.side2 = std::move(side2);
    s.mac = std::move(mac); s.mac2 = std::move(mac2);
    s.done[0] = std::move(done[0]); s.done[1] = std::move(done[1]);
    s.counted += 2 * 16 * sizeof(float) + 2 * 2 * sizeof(double);
    return true;
}

// a work list replaced as set_items replaces one: the new list is a local until it exists
bool replace_items(Dev<int> &items, size_t &n_items, size_t n)
{
    Dev<int> made;
    if (made.alloc(n)) return false;
    items = std::move(made);
    n_items = n;
    return true;
}

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { printf("FAILED at position %d: %s\n", g_fail_at, #cond); return 1; }      \
    } while (0)

void start(int fail_at) { g_calls = 0; g_fail_at = fail_at; g_live = 0; g_released = 0; }

}  // namespace

int main()
{
    for (int fail_at = -1; fail_at < 6; ++fail_at) {
        start(fail_at);
        {
            Set s;
            const bool made = make_set(s);
            if (fail_at < 0) {
                CHECK(made && s.side && s.side2 && s.mac && s.mac2 && s.done[0] && s.done[1] && g_live == 6 && g_calls == 6 && s.counted == 160);
            } else {
                CHECK(!made);
                CHECK(!s.side && !s.side2 && !s.mac && !s.mac2 && !s.done[0] && !s.done[1]);
                CHECK(g_live == 0 && s.counted == 0);
                CHECK(g_calls == fail_at + 1);               // nothing is attempted after the failure
            }
        }
        CHECK(g_live == 0);
    }
    start(-1);
    {   // the destructor releases exactly once; reset() releases now, and on an empty object does nothing
        {
            Dev<float> a;
            Ev f;
            CHECK(a.alloc(8) == 0 && a && a.size() == 8 && f.create() == 0 && f && g_live == 2);
        }
        CHECK(g_live == 0 && g_released == 2);
        Dev<float> b;
        Ev e;
        b.reset(); e.reset();
        CHECK(!b && b.size() == 0 && !e && g_released == 2);
        CHECK(b.alloc(4) == 0);
        b.reset();
        CHECK(!b && b.size() == 0 && g_live == 0 && g_released == 3);
        b.reset();
        CHECK(g_released == 3 && b.alloc(0) == 0 && !b && g_calls == 3);       // no elements: null, and the runtime is not asked
    }
    start(-1);
    {   // move-assignment releases what the target held, and the source is null afterwards; so is the source of a move construction
        Dev<int> a, b;
        Ev e, f;
        CHECK(a.alloc(3) == 0 && b.alloc(5) == 0 && e.create() == 0 && f.create() == 0 && g_live == 4);
        int *const pb = b;
        Event *const pf = f;
        a = std::move(b);
        CHECK(g_live == 3 && g_released == 1 && a.get() == pb && a.size() == 5 && !b && b.size() == 0);
        Dev<int> c(std::move(a));
        CHECK(g_live == 3 && g_released == 1 && c.get() == pb && c.size() == 5 && !a && a.size() == 0);
        e = std::move(f);
        CHECK(g_live == 2 && g_released == 2 && e.get() == pf && !f);
    }
    CHECK(g_live == 0);
    start(1);
    {   // build-then-commit: a replacement whose allocation fails leaves the previous array and its count intact
        Dev<int> items;
        size_t n_items = 0;
        CHECK(replace_items(items, n_items, 7) && items && n_items == 7 && g_live == 1);
        int *const before = items;
        before[6] = 42;
        CHECK(!replace_items(items, n_items, 9));
        CHECK(items.get() == before && items.size() == 7 && n_items == 7 && before[6] == 42 && g_live == 1 && g_released == 0);
        CHECK(replace_items(items, n_items, 9) && items.size() == 9 && n_items == 9 && g_live == 1 && g_released == 1);
        // in place (buffers sized with a result): released first, so after a failure it is null and the runtime's code comes back
        g_fail_at = g_calls;
        CHECK(items.alloc(16) == 2 && !items && items.size() == 0 && g_live == 0 && g_released == 2);
    }
    CHECK(g_live == 0);
    printf("device memory OK: all-or-nothing at each of 6 positions, release once, move, reset, build-then-commit\n");
    return 0;
}
