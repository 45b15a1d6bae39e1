// devmem_harness.cpp — the two owners of f110_devmem.hpp on the CPU: the header's host seam (-DF110_DEVMEM_HOST: malloc / free and
// "fail the n-th allocation from now") under the address and undefined-behaviour sanitizers.  A stand-alone program: after every
// scenario the live and byte counters are back where they were before it, and a leak or a double free is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_devmem.hpp"

using devmem::DevArena;
using devmem::DevBuf;
using devmem::kOk;

static int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("devmem harness: line %d: %s\n", __LINE__, #cond);  \
            g_failed += 1;                                                  \
        }                                                                   \
    } while (0)

struct Counters {
    int64_t live, bytes;
    Counters() : live(devmem::g_live.load()), bytes(devmem::g_bytes.load()) {}
    bool back() const { return devmem::g_live.load() == live && devmem::g_bytes.load() == bytes; }
    bool grew_by(int64_t n, int64_t b) const { return devmem::g_live.load() == live + n && devmem::g_bytes.load() == bytes + b; }
};

// what the handle's slot vectors hold (MapSlot / TrackSlot): buffers next to plain fields
struct Slot {
    DevBuf<double> table, pad;
    DevBuf<unsigned char> occ;
    int tag = 0;
};

static void buf_scenarios()
{
    const Counters c0;
    {
        DevBuf<double> b;
        CHECK(!b && b.get() == nullptr && b.capacity() == 0);
        CHECK(b.alloc(10) == kOk && b && b.capacity() == 10 && c0.grew_by(1, 80));
        std::memset(b, 0, 80);   // (the conversion to T *; the sanitizer checks the extent)
        b[9] = 1.0;
        double *first = b;
        CHECK(b.alloc(20) == kOk && b.capacity() == 20 && c0.grew_by(1, 160));   // re-alloc frees what it held
        (void)first;
        b[19] = 2.0;
        double *held = b;
        CHECK(b.grow(5) == kOk && b.get() == held && b.capacity() == 20);    // below the capacity
        CHECK(b.grow(20) == kOk && b.get() == held && b.capacity() == 20);   // at it
        CHECK(b.grow(21) == kOk && b.capacity() == 21 && c0.grew_by(1, 168));   // above: a new allocation
        b[20] = 3.0;
        b.reset();
        CHECK(!b && b.capacity() == 0 && c0.back());
        b.reset();   // twice is harmless
        CHECK(b.grow(0) == kOk && b && c0.grew_by(1, 8));   // a zero count still yields a pointer of its own
        CHECK(b.alloc(0) == kOk && b && b.capacity() == 0 && c0.grew_by(1, 8));
        CHECK(b.grow(0) == kOk && c0.grew_by(1, 8));
    }
    CHECK(c0.back());
    {   // moves
        DevBuf<int> a;
        CHECK(a.alloc(7) == kOk);
        int *pa = a;
        DevBuf<int> b(std::move(a));
        CHECK(!a && a.capacity() == 0 && b.get() == pa && b.capacity() == 7 && c0.grew_by(1, 28));
        DevBuf<int> live;
        CHECK(live.alloc(3) == kOk && c0.grew_by(2, 40));
        live = std::move(b);   // onto a live buffer: its old allocation goes
        CHECK(!b && live.get() == pa && live.capacity() == 7 && c0.grew_by(1, 28));
        live[6] = 5;
        DevBuf<int> &self = live;
        live = std::move(self);   // self-assignment keeps it
        CHECK(live.get() == pa && live.capacity() == 7 && c0.grew_by(1, 28));
        CHECK(a.alloc(2) == kOk && a.capacity() == 2 && c0.grew_by(2, 36));   // a moved-from buffer is an empty one
        live = DevBuf<int>();   // how a field is cleared by assignment
        CHECK(!live && c0.grew_by(1, 8));
    }
    CHECK(c0.back());
    {   // a failed allocation: what was held is gone, the buffer is empty and usable
        DevBuf<float> b;
        CHECK(b.alloc(4) == kOk);
        devmem::fail_nth(1);
        CHECK(b.alloc(8) != kOk && !b && b.capacity() == 0 && c0.back());
        CHECK(b.grow(8) == kOk && b.capacity() == 8);
        devmem::fail_nth(1);
        CHECK(b.grow(4) == kOk);   // no allocation: the failure stays pending ...
        CHECK(b.grow(16) != kOk && !b && c0.back());   // ... for this one
    }
    CHECK(c0.back());
}

static void vector_scenario()
{
    const Counters c0;
    {
        std::vector<Slot> slots;
        std::vector<const double *> tables;
        for (int i = 0; i < 37; ++i) {   // well past any first capacity: the vector reallocates and MOVES its slots
            Slot s;
            CHECK(s.table.alloc((size_t)i + 1) == kOk && s.pad.alloc(2 * (size_t)i) == kOk);
            if (i % 3 == 0) CHECK(s.occ.alloc(5) == kOk);
            s.table[i] = i;
            s.tag = i;
            tables.push_back(s.table);
            slots.push_back(std::move(s));
            CHECK(!s.table && !s.pad && !s.occ);
        }
        for (int i = 0; i < 37; ++i) CHECK(slots[i].tag == i && slots[i].table.get() == tables[i] && slots[i].table[i] == i);
        CHECK(c0.grew_by(37 * 2 + 13, devmem::g_bytes.load() - c0.bytes));
        slots.pop_back();   // (the failure path of f110_add_map_obstacles)
        CHECK(c0.grew_by(36 * 2 + 13 - 1, devmem::g_bytes.load() - c0.bytes));
        slots.resize(40);   // (f110_track_set's resize: empty slots)
        CHECK(!slots[39].table);
        slots[2] = Slot{};
        CHECK(!slots[2].table && slots[3].table);
    }
    CHECK(c0.back());
}

// what a kernel takes by value: raw pointers, owned by an arena next to it
struct Job {
    double *a = nullptr, *b = nullptr;
    int *c = nullptr;
    unsigned char *d = nullptr;
    long long *e = nullptr;
};

static devmem::err_t fill(DevArena &m, Job &j)
{
    devmem::err_t e = m.alloc(&j.a, 3);
    if (e == kOk) e = m.alloc(&j.b, 100);
    if (e == kOk) e = m.alloc(&j.c, 0);
    if (e == kOk) e = m.alloc(&j.d, 7);
    if (e == kOk) e = m.alloc(&j.e, 2);
    return e;
}

static void arena_scenarios()
{
    const Counters c0;
    const int64_t all = 24 + 800 + 8 + 7 + 16;
    {
        DevArena m;
        Job j;
        CHECK(fill(m, j) == kOk && m.size() == 5 && c0.grew_by(5, all));
        CHECK(j.a && j.b && j.c && j.d && j.e);   // the zero count too
        j.b[99] = 1.0;
        j.d[6] = 1;
        m.clear();
        CHECK(m.size() == 0 && c0.back());
        m.clear();
        j = Job{};
        CHECK(fill(m, j) == kOk && c0.grew_by(5, all));   // (disarm, arm again)
        DevArena n(std::move(m));
        CHECK(m.size() == 0 && n.size() == 5 && c0.grew_by(5, all));
        j.e[1] = 7;   // the pointers stay good across the move
        DevArena o;
        double *x = nullptr;
        CHECK(o.alloc(&x, 1) == kOk && c0.grew_by(6, all + 8));
        o = std::move(n);   // onto a live arena: its allocations go
        CHECK(n.size() == 0 && o.size() == 5 && c0.grew_by(5, all));
        DevArena &self = o;
        o = std::move(self);
        CHECK(o.size() == 5 && c0.grew_by(5, all));
    }
    CHECK(c0.back());
    for (int n = 1; n <= 5; ++n) {   // "built aside": the n-th of the five allocations fails, the local is dropped
        {
            DevArena aside;
            Job j;
            devmem::fail_nth(n);
            CHECK(fill(aside, j) != kOk && aside.size() == (size_t)n - 1 && devmem::g_live.load() == c0.live + n - 1);
        }
        CHECK(c0.back());
        {   // the same with buffers as members (f110_sim::Mppi / Pf)
            struct Built {
                DevBuf<double> a, b;
                DevBuf<int> c;
                DevBuf<unsigned char> d;
                DevBuf<long long> e;
            } aside, armed;
            CHECK(armed.a.alloc(1) == kOk);
            devmem::fail_nth(n);
            devmem::err_t e = aside.a.alloc(3);
            if (e == kOk) e = aside.b.alloc(100);
            if (e == kOk) e = aside.c.alloc(0);
            if (e == kOk) e = aside.d.alloc(7);
            if (e == kOk) e = aside.e.alloc(2);
            CHECK(e != kOk && armed.a && devmem::g_live.load() == c0.live + n);   // what is armed stays as it is
        }
        CHECK(c0.back());
    }
    devmem::fail_nth(6);
    {
        DevArena m;
        Job j;
        CHECK(fill(m, j) == kOk);   // the sixth allocation is not one of these five
        devmem::fail_nth(0);
    }
    CHECK(c0.back());
}

int main()
{
    buf_scenarios();
    vector_scenario();
    arena_scenarios();
    if (g_failed || devmem::g_live.load() != 0 || devmem::g_bytes.load() != 0) {
        std::printf("devmem harness: %d checks failed, %lld allocations / %lld bytes live at the end\n", g_failed, (long long)devmem::g_live.load(),
                    (long long)devmem::g_bytes.load());
        return 1;
    }
    std::printf("devmem harness: ok\n");
    return 0;
}
