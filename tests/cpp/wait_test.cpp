// The host half of the publication protocol (csrc/re_wait.h) without a device: the bounded poll of a published word, the seal settle, and the
// waits composed of them (wait_word, wait_sealed).
// Built with plain g++ and the standard library only.  With -DRE_TEST_SEALS (which needs the HIP headers for re_kernels.h) it also pins
// the seal and sign-off formulas the kernels and the host share.  Only lower bounds on elapsed time are asserted: machines stall.
#include "re_wait.h"
#ifdef RE_TEST_SEALS
#include "re_kernels.h"
#endif
#include <cstdio>
#include <thread>

using namespace re;
using clk = std::chrono::steady_clock;
using std::chrono::milliseconds;
using std::chrono::seconds;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static void poll_cases() {
    {   // already equal: true at once
        uint32_t word = 7;
        CHECK(poll_word(&word, 7u, milliseconds(1)));
    }
    {   // never equal: false, and not before the limit
        uint32_t word = 7;
        const auto t0 = clk::now();
        CHECK(!poll_word(&word, 8u, milliseconds(2)));
        CHECK(clk::now() - t0 >= milliseconds(2));
    }
    {   // a writer publishes a payload and then the word: the payload read behind the poll is the written one
        uint32_t word = 0, payload[16] = {};
        std::thread writer([&] {
            std::this_thread::sleep_for(milliseconds(1));
            for (uint32_t i = 0; i < 16; i++) payload[i] = 0xC0DE0000u + i;
            __atomic_store_n(&word, 5u, __ATOMIC_RELEASE);
        });
        const bool seen = poll_word(&word, 5u, seconds(1));
        bool whole = true;
        for (uint32_t i = 0; i < 16; i++) whole = whole && payload[i] == 0xC0DE0000u + i;
        writer.join();
        CHECK(seen); CHECK(whole);
    }
}

// a block that agrees on its k-th look (k == 0: never), or once the synchronise has run
struct Block {
    uint32_t agrees_on = 0, looks = 0, syncs = 0; bool agrees_after_sync = false;
    bool sealed() { looks++; return (agrees_on && looks >= agrees_on) || (agrees_after_sync && syncs); }
};
static void settle_cases() {
    const uint32_t W = 10, F = 20;           // the counters are the caller's: the settle only adds to them
    {   // first look: nothing counted, no synchronise
        Block b; b.agrees_on = 1; uint32_t waits = W, fallbacks = F;
        CHECK(settle_seal([&] { return b.sealed(); }, milliseconds(2), waits, fallbacks, [&] { b.syncs++; }) == Seal::at_first_sight);
        CHECK(waits == W && fallbacks == F && b.syncs == 0 && b.looks == 1);
    }
    {   // a later look within the limit (the second: no clock reading lies in front of it)
        Block b; b.agrees_on = 2; uint32_t waits = W, fallbacks = F;
        CHECK(settle_seal([&] { return b.sealed(); }, milliseconds(2), waits, fallbacks, [&] { b.syncs++; }) == Seal::after_wait);
        CHECK(waits == W + 1 && fallbacks == F && b.syncs == 0);
    }
    {   // only after the synchronise
        Block b; b.agrees_after_sync = true; uint32_t waits = W, fallbacks = F;
        const auto t0 = clk::now();
        CHECK(settle_seal([&] { return b.sealed(); }, milliseconds(1), waits, fallbacks, [&] { b.syncs++; }) == Seal::after_sync);
        CHECK(clk::now() - t0 >= milliseconds(1));
        CHECK(waits == W + 1 && fallbacks == F + 1 && b.syncs == 1);
    }
    {   // never
        Block b; uint32_t waits = W, fallbacks = F;
        const auto t0 = clk::now();
        CHECK(settle_seal([&] { return b.sealed(); }, milliseconds(1), waits, fallbacks, [&] { b.syncs++; }) == Seal::never);
        CHECK(clk::now() - t0 >= milliseconds(1));
        CHECK(waits == W + 1 && fallbacks == F + 1 && b.syncs == 1);
    }
    {   // never, and the caller has no synchronise (finish_tick)
        Block b; uint32_t waits = W, fallbacks = F;
        CHECK(settle_seal([&] { return b.sealed(); }, milliseconds(1), waits, fallbacks) == Seal::never);
        CHECK(waits == W + 1 && fallbacks == F + 1);
    }
}

// a synchronise that counts its calls and fails (returns `code`) at its fail_on-th
struct CountedSync {
    Block &b; uint32_t fail_on = 0; int code = -7;
    int operator()() { b.syncs++; return b.syncs == fail_on ? code : 0; }
};
static void wait_cases() {
    const uint32_t W = 10, F = 20;
    {   // wait_word: the word is there (no synchronise); the word never comes (one synchronise, 0); that synchronise fails (its code)
        Block b; uint32_t word = 3;
        CHECK(wait_word(&word, 3u, milliseconds(1), CountedSync{ b }) == 0 && b.syncs == 0);
        const auto t0 = clk::now();
        CHECK(wait_word(&word, 4u, milliseconds(1), CountedSync{ b }) == 0 && b.syncs == 1);
        CHECK(clk::now() - t0 >= milliseconds(1));
        Block b2;
        CHECK(wait_word(&word, 4u, milliseconds(1), CountedSync{ b2, 1 }) == -7 && b2.syncs == 1);
    }
    {   // the word in time (from a writer thread, behind the block it guards), the seal agrees: no synchronise, nothing counted
        Block b; b.agrees_on = 1; uint32_t waits = W, fallbacks = F, word = 0, payload = 0;
        std::thread writer([&] { std::this_thread::sleep_for(milliseconds(1)); payload = 0xC0DEu; __atomic_store_n(&word, 5u, __ATOMIC_RELEASE); });
        const int rc = wait_sealed(&word, 5u, seconds(1), [&] { return b.sealed() && payload == 0xC0DEu; }, milliseconds(1), waits, fallbacks, CountedSync{ b });
        writer.join();
        CHECK(rc == 0 && b.syncs == 0 && b.looks == 1 && waits == W && fallbacks == F);
    }
    {   // the word never arrives: exactly one synchronise, then the seal is looked at (and agrees: the stream has ended)
        Block b; b.agrees_after_sync = true; uint32_t waits = W, fallbacks = F, word = 0;
        const auto t0 = clk::now();
        CHECK(wait_sealed(&word, 5u, milliseconds(1), [&] { return b.sealed(); }, milliseconds(1), waits, fallbacks, CountedSync{ b }) == 0);
        CHECK(clk::now() - t0 >= milliseconds(1));
        CHECK(b.syncs == 1 && b.looks == 1 && waits == W && fallbacks == F);
    }
    {   // ... and that synchronise fails: failure at once, the seal is never looked at, nothing counted
        Block b; b.agrees_on = 1; uint32_t waits = W, fallbacks = F, word = 0;
        CHECK(wait_sealed(&word, 5u, milliseconds(1), [&] { return b.sealed(); }, milliseconds(1), waits, fallbacks, CountedSync{ b, 1 }) == -7);
        CHECK(b.syncs == 1 && b.looks == 0 && waits == W && fallbacks == F);
    }
    {   // the word arrives, the seal never agrees: one seal wait, one fallback with its one synchronise -- and success (the caller reads the block behind the synchronise)
        Block b; uint32_t waits = W, fallbacks = F, word = 5;
        const auto t0 = clk::now();
        CHECK(wait_sealed(&word, 5u, milliseconds(1), [&] { return b.sealed(); }, milliseconds(1), waits, fallbacks, CountedSync{ b }) == 0);
        CHECK(clk::now() - t0 >= milliseconds(1));
        CHECK(b.syncs == 1 && waits == W + 1 && fallbacks == F + 1);
    }
    {   // ... and the fallback's synchronise fails: failure
        Block b; uint32_t waits = W, fallbacks = F, word = 5;
        CHECK(wait_sealed(&word, 5u, milliseconds(1), [&] { return b.sealed(); }, milliseconds(1), waits, fallbacks, CountedSync{ b, 1 }) == -7);
        CHECK(b.syncs == 1 && waits == W + 1 && fallbacks == F + 1);
    }
    {   // the poll times out, its synchronise succeeds, the seal still disagrees and the fallback's synchronise (the second) fails: failure
        Block b; uint32_t waits = W, fallbacks = F, word = 0;
        CHECK(wait_sealed(&word, 5u, milliseconds(1), [&] { return b.sealed(); }, milliseconds(1), waits, fallbacks, CountedSync{ b, 2 }) == -7);
        CHECK(b.syncs == 2 && waits == W + 1 && fallbacks == F + 1);
    }
}

#ifdef RE_TEST_SEALS
// the two-level sign-off (list_sign_off, re_kernels.h): every participant is expected by exactly one shard, the top counter expects exactly the shards
// that expect anybody, and no participant signs a counter that expects nobody
static void signoff_cases(uint32_t total) {
    const uint32_t S = LOGIC_TICKET_SHARDS;
    uint32_t sum = 0, nonzero = 0;
    for (uint32_t sh = 0; sh < S; sh++) { const uint32_t e = signoff_expect(total, sh, S); sum += e; nonzero += e != 0u; }
    CHECK(sum == total);
    CHECK(nonzero == signoff_top(total, S));
    bool all = true;
    for (uint32_t i = 0; i < total && i < 4096u; i++) all = all && signoff_expect(total, i & (S - 1u), S) > 0u;
    CHECK(all);
}
static void seal_cases() {
    const uint32_t v[] = { 0u, 1u, 2u, 255u, 65536u, 0x12345678u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu };
    const uint32_t n = sizeof v / sizeof v[0];
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t a = v[i], b = v[(i + 1) % n], c = v[(i + 3) % n], d = v[(i + 4) % n], e = v[(i + 5) % n], f = v[(i + 7) % n], g = v[(i + 8) % n];
        CHECK(tick_seal(a, b, c, d) == (table_word_hash(a, 1u) ^ table_word_hash(b, 2u) ^ table_word_hash(c, 3u) ^ table_word_hash(d, 4u)));
        CHECK(col_seal(a, b, c, d, e, f, g) == (table_word_hash(a, 1u) ^ table_word_hash(b, 2u) ^ table_word_hash(c, 3u) ^ table_word_hash(d, 4u) ^ table_word_hash(e, 5u) ^
                                                table_word_hash(f, 6u) ^ table_word_hash(g, 7u)));
        CHECK(logic_seal(a, b) == (table_word_hash(a, 1u) ^ table_word_hash(b, 2u)));
        CHECK(tick_seal(a, a, a, a) == (table_word_hash(a, 1u) ^ table_word_hash(a, 2u) ^ table_word_hash(a, 3u) ^ table_word_hash(a, 4u)));
    }
    // the hash itself, so that the pins above do not move with it: (v ^ w * 0x9E3779B1) * 0x85EBCA6B, folded by 15 bits
    CHECK(table_word_hash(0u, 0u) == 0u);
    { const uint32_t x = (0xFFFFFFFFu ^ (4u * 0x9E3779B1u)) * 0x85EBCA6Bu; CHECK(table_word_hash(0xFFFFFFFFu, 4u) == (x ^ (x >> 15))); }
    CHECK(tick_seal(1u, 2u, 3u, 4u) != tick_seal(2u, 1u, 3u, 4u));           // the salts tie a value to its place
    static_assert(LOGIC_TICKET_SHARDS == 32u, "the sign-off cases below are the issue's: 32 shards");
    for (uint32_t total = 1; total <= 200u; total++) signoff_cases(total);
    signoff_cases((1u << 20) + 1u);
}
#endif

int main() {
    poll_cases();
    settle_cases();
    wait_cases();
#ifdef RE_TEST_SEALS
    seal_cases();
#endif
    if (failures) return 1;
    puts("ok");
    return 0;
}
