// Host check of lw::make_all_or_nothing (open_ludwig_amd/csrc/all_or_nothing.hpp), the rule the second set of interface side buffers
// is made by: four buffers and two events, all of them or none. The allocator is a stand-in that fails at a chosen call; a failure is
// injected at each of the six positions in turn. tests/test_library_abi.py builds it with -fsanitize=address,undefined, so leaks and double frees are reported too.
#include <cstdio>
#include <cstdlib>

#include "all_or_nothing.hpp"

namespace {

struct Event { int id; };

int g_calls = 0, g_fail_at = -1, g_live = 0;

bool fake_alloc(void **p, size_t n)
{
    if (g_calls++ == g_fail_at) { *p = reinterpret_cast<void *>(0x1); return false; }     // a failed call may leave rubbish behind
    *p = malloc(n);
    ++g_live;
    return true;
}
void fake_free(void *p) { free(p); --g_live; }
bool fake_create(Event **e)
{
    if (g_calls++ == g_fail_at) return false;
    *e = new Event{g_calls};
    ++g_live;
    return true;
}
void fake_destroy(Event *e) { delete e; --g_live; }

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { printf("FAILED at position %d: %s\n", g_fail_at, #cond); return 1; }      \
    } while (0)

}  // namespace

int main()
{
    for (int fail_at = -1; fail_at < 6; ++fail_at) {
        void *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
        Event *e0 = nullptr, *e1 = nullptr;
        void **const bufs[4] = {&a, &b, &c, &d};
        const size_t bytes[4] = {64, 64, 16, 16};
        Event **const evs[2] = {&e0, &e1};
        long counted = 0;
        g_calls = 0; g_fail_at = fail_at; g_live = 0;
        const bool made = lw::make_all_or_nothing(bufs, bytes, evs, fake_alloc, fake_free, fake_create, fake_destroy);
        if (made) counted += 64 + 64 + 16 + 16;
        if (fail_at < 0) {
            CHECK(made && a && b && c && d && e0 && e1 && g_live == 6 && g_calls == 6 && counted == 160);
            for (void **q : bufs) fake_free(*q);
            fake_destroy(e0); fake_destroy(e1);
        } else {
            CHECK(!made);
            CHECK(!a && !b && !c && !d && !e0 && !e1);
            CHECK(g_live == 0 && counted == 0);
            CHECK(g_calls == fail_at + 1);               // nothing is attempted after the failure
        }
        CHECK(g_live == 0);
    }
    printf("all-or-nothing OK: success and a failure at each of 6 positions\n");
    return 0;
}
