// re_wait.h -- the host half of the publication protocol (the device half is publish_to_host, re_kernels.h): how the
// host thread waits for a block a kernel writes into mapped host memory, and how far it believes the block.  Host only, standard library only.
#pragma once
#include <atomic>
#include <chrono>
#include <stdint.h>

namespace re {

// Spins until the published word equals `want`; false once `limit` has passed (the caller then lets the driver wait).  The clock is read every
// 1024th spin only: it costs more than the read of the word.  The acquire fence in front of `true` orders the reads of the block behind the word.
inline bool poll_word(const volatile uint32_t *word, uint32_t want, std::chrono::steady_clock::duration limit) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; *word != want; spins++)
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > limit) return false;
    std::atomic_thread_fence(std::memory_order_acquire);
    return true;
}

// The seal of a block whose word has arrived.  With publish_to_host it agrees at first sight and nothing is counted.  Otherwise: one seal wait
// and up to `limit` of re-checks; then one sync fallback, the caller's synchronise (if it has one), a fence and a last check.
enum class Seal { at_first_sight, after_wait, after_sync, never };
struct NoSync { void operator()() const {} };
template <typename Sealed, typename Sync = NoSync>
inline Seal settle_seal(Sealed &&sealed, std::chrono::steady_clock::duration limit, uint32_t &n_seal_waits, uint32_t &n_sync_fallbacks, Sync &&sync = Sync{}) {
    if (sealed()) return Seal::at_first_sight;
    n_seal_waits++;
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = false;
    while (!(ok = sealed()) && std::chrono::steady_clock::now() - t0 < limit) {}
    if (ok) return Seal::after_wait;
    n_sync_fallbacks++;
    sync();
    std::atomic_thread_fence(std::memory_order_acquire);
    return sealed() ? Seal::after_sync : Seal::never;
}

// "Poll, else synchronise and fence", for a word with no seal behind it.  `sync` is the caller's synchronise, 0 when it succeeded; returns 0, or what `sync` returned.
template <typename Sync>
inline int wait_word(const volatile uint32_t *word, uint32_t want, std::chrono::steady_clock::duration poll_limit, Sync &&sync) {
    if (poll_word(word, want, poll_limit)) return 0;
    if (const int rc = sync()) return rc;
    std::atomic_thread_fence(std::memory_order_acquire);
    return 0;
}

// The whole wait for a sealed block: the word, then the seal.  A failed synchronise ends it at once -- no look at the seal, no counter touched.
// After a synchronise that succeeded the stream's end is authoritative: the caller reads the block whatever the seal says.
template <typename Sealed, typename Sync>
inline int wait_sealed(const volatile uint32_t *word, uint32_t want, std::chrono::steady_clock::duration poll_limit, Sealed &&sealed, std::chrono::steady_clock::duration seal_limit, uint32_t &n_seal_waits, uint32_t &n_sync_fallbacks, Sync &&sync) {
    int rc = wait_word(word, want, poll_limit, sync);
    if (rc == 0) settle_seal(sealed, seal_limit, n_seal_waits, n_sync_fallbacks, [&] { rc = sync(); });
    return rc;
}

}  // namespace re
