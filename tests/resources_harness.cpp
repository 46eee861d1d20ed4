// CPU harness for active-gym_amd/csrc/agx_resources.h with a mocked runtime (no HIP): the block layouts of the six handles on the
// frame history, and the owner's bookkeeping when the k-th acquisition of a create fails - the paths a GPU test cannot reach
// without provoking an allocation failure.  The mock's memory is real malloc memory, so under -fsanitize=address a block the
// owner forgets or frees twice is the sanitizer's finding as well.  Prints "ok" or the first failed check.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "agx_resources.h"

namespace {

enum Kind { kDev, kPin, kEv, kSt };
struct Live {
    Kind kind;
    int device;      // the device that was current when it was made
};
std::map<void *, Live> g_live;
int g_cur = 0, g_ndev = 8;
bool g_set_fails = false;
std::vector<int> g_sets;
int g_calls = 0, g_fail_at = -1;          // the g_fail_at-th acquisition (1-based) is refused with kRefused
int g_frees = 0, g_bad_frees = 0, g_frees_off_device = 0, g_free_device = -1;
unsigned g_last_flags = 0;
int g_last_priority = 0;
constexpr int kRefused = 77;

struct MockApi {
    using Error = int;
    static int get(int *d) {
        *d = g_cur;
        return 0;
    }
    static int set(int d) {
        g_sets.push_back(d);
        if (g_set_fails || d < 0 || d >= g_ndev) return 1;
        g_cur = d;
        return 0;
    }
    static Error make(void **p, Kind kind, size_t bytes) {
        if (++g_calls == g_fail_at) return kRefused;
        *p = bytes ? malloc(bytes) : nullptr;
        if (*p) g_live[*p] = Live{kind, g_cur};
        return 0;
    }
    static void drop(void *p, Kind kind) {
        ++g_frees;
        if (g_free_device >= 0 && g_cur != g_free_device) ++g_frees_off_device;
        auto it = g_live.find(p);
        if (it == g_live.end() || it->second.kind != kind) {      // unknown, already freed, or freed as another kind
            ++g_bad_frees;
            return;
        }
        g_live.erase(it);
        free(p);
    }
    static Error device_alloc(void **p, size_t bytes) { return make(p, kDev, bytes); }
    static void device_free(void *p) { drop(p, kDev); }
    static Error pinned_alloc(void **p, size_t bytes) { return make(p, kPin, bytes); }
    static void pinned_free(void *p) { drop(p, kPin); }
    static Error event_create(void **e, unsigned flags) {
        g_last_flags = flags;
        return make(e, kEv, 1);
    }
    static void event_destroy(void *e) { drop(e, kEv); }
    static Error stream_create(void **s, unsigned flags) {
        g_last_flags = flags;
        return make(s, kSt, 1);
    }
    static Error stream_create_priority(void **s, unsigned flags, int priority) {
        g_last_flags = flags;
        g_last_priority = priority;
        return make(s, kSt, 1);
    }
    static void stream_destroy(void *s) { drop(s, kSt); }
};
using Owner = agx::ResourcesT<MockApi>;
struct Event;       // opaque handle types, as the runtime's are
struct Stream;

#define CHECK(c)                                  \
    do {                                          \
        if (!(c)) {                               \
            printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            return 1;                             \
        }                                         \
    } while (0)

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }       // hist_align of the commit before agx_resources.h

// What a create does: eight acquisitions of mixed kinds, leaving at the first refusal with the runtime's code
struct Handle {
    explicit Handle(int device) : own(device) {}
    Owner own;
    uint8_t *d0 = nullptr, *d1 = nullptr, *h0 = nullptr;
    float *h1 = nullptr;
    Event *e0 = nullptr, *e1 = nullptr;
    Stream *s0 = nullptr, *s1 = nullptr;
};
constexpr int kSteps = 8;
int build(Handle *h) {
    int e;
    if ((e = h->own.device_mem(&h->d0, 1000))) return e;
    if ((e = h->own.pinned(&h->h0, 64))) return e;
    if ((e = h->own.event(&h->e0, 2u))) return e;
    if ((e = h->own.stream(&h->s0, 1u))) return e;
    if ((e = h->own.device_mem(&h->d1, 3))) return e;
    if ((e = h->own.stream(&h->s1, 1u, -1))) return e;
    if ((e = h->own.pinned(&h->h1, 4 * sizeof(float)))) return e;
    if ((e = h->own.event(&h->e1, 2u))) return e;
    return 0;
}
int made(const Handle &h) {
    const void *p[kSteps] = {h.d0, h.h0, h.e0, h.s0, h.d1, h.s1, h.h1, h.e1};
    int n = 0;
    for (const void *q : p) n += q != nullptr;
    return n;
}
void reset_counters() {
    g_calls = g_frees = g_bad_frees = g_frees_off_device = 0;
    g_fail_at = g_free_device = -1;
    g_sets.clear();
}

}  // namespace

int main() {
    // ---- layout: offsets are the running sum of the 256-padded sizes; a zero-byte section takes no space
    {
        agx::BlockLayout lay;
        CHECK(lay.bytes() == 0);
        CHECK(lay.add(1) == 0 && lay.bytes() == 256);
        CHECK(lay.add(256) == 256 && lay.bytes() == 512);
        CHECK(lay.add(0) == 512 && lay.bytes() == 512);
        CHECK(lay.add(257) == 512 && lay.bytes() == 1024);
        CHECK(lay.add(((size_t)5 << 32) + 3) == 1024 && lay.bytes() == 1024 + ((size_t)5 << 32) + 256);     // (past 4 GiB)
        uint8_t block[8];
        CHECK(reinterpret_cast<uint8_t *>(agx::BlockLayout::at<int64_t>(block, 4)) == block + 4);
        for (size_t b : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)105840}) CHECK(agx::BlockLayout::pad(b) == al(b));
    }
    // ---- the six handles' section lists at N = 3, T = 5, one 84 x 84 plane, payload 12, back / forward irrelevant, against the
    // formulas of the commit before (b_* sums of hist_align terms, written out here as they stood):
    //   history 106752   replay 512   step log 1024   priorities 2560   shifts 256   minibatches 768
    {
        const size_t N = 3, T = 5, fbytes = 84 * 84, W = 12, rows = T * N;
        const size_t CH = (T + 64 - 1) / 64, chunks = N * CH;             // kPrioChunk = 64 (agx_k9_priority.h)
        agx::BlockLayout hist, replay, steplog, prio, shift, mb;
        size_t o[10];
        // agx_history_create: frames | loc | count | age
        o[0] = hist.add(T * N * fbytes), o[1] = hist.add(T * N * 2 * sizeof(int32_t)), o[2] = hist.add(N * sizeof(int64_t)), o[3] = hist.add(T * N);
        const size_t b_frames = al(T * N * fbytes), b_loc = al(T * N * 2 * sizeof(int32_t)), b_count = al(N * sizeof(int64_t)), b_age = al(T * N);
        CHECK(hist.bytes() == b_frames + b_loc + b_count + b_age && hist.bytes() == 106752);
        CHECK(o[0] == 0 && o[1] == b_frames && o[2] == b_frames + b_loc && o[3] == b_frames + b_loc + b_count);
        // agx_replay_create: off | state
        o[0] = replay.add((N + 1) * sizeof(int64_t)), o[1] = replay.add(3 * sizeof(uint64_t));
        CHECK(replay.bytes() == al((N + 1) * sizeof(int64_t)) + al(3 * sizeof(uint64_t)) && replay.bytes() == 512 && o[1] == al((N + 1) * sizeof(int64_t)));
        // agx_steplog_create: stamp | reward | flags | payload
        o[0] = steplog.add(rows * sizeof(int64_t)), o[1] = steplog.add(rows * sizeof(float)), o[2] = steplog.add(rows), o[3] = steplog.add(rows * W);
        const size_t b_stamp = al(rows * sizeof(int64_t)), b_reward = al(rows * sizeof(float)), b_flags = al(rows), b_payload = al(rows * W);
        CHECK(steplog.bytes() == b_stamp + b_reward + b_flags + b_payload && steplog.bytes() == 1024);
        CHECK(o[1] == b_stamp && o[2] == b_stamp + b_reward && o[3] == b_stamp + b_reward + b_flags);
        // agx_priority_create: stamp | incl | csum | envsum | envacc | off | state | weight | cacc | wmax
        o[0] = prio.add(rows * sizeof(int64_t)), o[1] = prio.add(rows * sizeof(int64_t)), o[2] = prio.add(chunks * sizeof(int64_t));
        o[3] = prio.add(N * sizeof(int64_t)), o[4] = prio.add(N * sizeof(int64_t)), o[5] = prio.add((N + 1) * sizeof(int64_t));
        o[6] = prio.add(3 * sizeof(uint64_t)), o[7] = prio.add(rows * sizeof(uint32_t)), o[8] = prio.add(chunks * sizeof(int32_t)), o[9] = prio.add(sizeof(uint32_t));
        const size_t p_stamp = al(rows * sizeof(int64_t)), p_incl = p_stamp, p_csum = al(chunks * sizeof(int64_t)), p_env = al(N * sizeof(int64_t)),
                     p_off = al((N + 1) * sizeof(int64_t)), p_state = al(3 * sizeof(uint64_t)), p_weight = al(rows * sizeof(uint32_t)),
                     p_cacc = al(chunks * sizeof(int32_t)), p_wmax = al(sizeof(uint32_t));
        CHECK(prio.bytes() == p_stamp + p_incl + p_csum + 2 * p_env + p_off + p_state + p_weight + p_cacc + p_wmax && prio.bytes() == 2560);
        const size_t want[10] = {0, p_stamp, p_stamp + p_incl, p_stamp + p_incl + p_csum, p_stamp + p_incl + p_csum + p_env,
                                 p_stamp + p_incl + p_csum + 2 * p_env, p_stamp + p_incl + p_csum + 2 * p_env + p_off,
                                 p_stamp + p_incl + p_csum + 2 * p_env + p_off + p_state, p_stamp + p_incl + p_csum + 2 * p_env + p_off + p_state + p_weight,
                                 prio.bytes() - p_wmax};
        for (int k = 0; k < 10; ++k) CHECK(o[k] == want[k]);
        // agx_shift_create: state (kShiftStateBytes = 256)
        CHECK(shift.add(3 * sizeof(uint64_t)) == 0 && shift.bytes() == 256);
        // agx_minibatch_create: off | cnt | state
        o[0] = mb.add(2 * (N + 1) * sizeof(int32_t)), o[1] = mb.add(N * sizeof(int32_t)), o[2] = mb.add(6 * sizeof(uint64_t));
        const size_t m_off = al(2 * (N + 1) * sizeof(int32_t)), m_cnt = al(N * sizeof(int32_t)), m_state = al(6 * sizeof(uint64_t));
        CHECK(mb.bytes() == m_off + m_cnt + m_state && mb.bytes() == 768 && o[1] == m_off && o[2] == m_off + m_cnt);
    }
    // ---- failure injection: the k-th of the eight acquisitions is refused, for every k.  What was acquired before goes back
    // exactly once when the handle is deleted, nothing else does, and the caller saw the runtime's code.
    void *bystander = nullptr;                      // somebody else's allocation: never the owner's to free
    CHECK(MockApi::device_alloc(&bystander, 16) == 0);
    for (int k = 1; k <= kSteps; ++k) {
        reset_counters();
        g_fail_at = k;
        Handle *h = new Handle(0);
        CHECK(build(h) == kRefused);
        CHECK(g_calls == k && made(*h) == k - 1);                   // it stopped there, and the refused call left its pointer alone
        CHECK((int)g_live.size() == 1 + (k - 1) && g_frees == 0);
        delete h;
        CHECK(g_frees == k - 1 && g_bad_frees == 0);
        CHECK(g_live.size() == 1 && g_live.count(bystander) == 1);
    }
    // ---- full success: flags and priority reach the runtime; release() gives all eight back, a second release() and the
    // destructor nothing more; the owner works again after a release
    {
        reset_counters();
        Handle *h = new Handle(0);
        CHECK(build(h) == 0 && made(*h) == kSteps && g_live.size() == 1 + kSteps);
        CHECK(g_last_flags == 2u && g_last_priority == -1);
        h->h1[3] = 1.0f;                                            // (the memory is the caller's to use)
        h->own.release();
        CHECK(g_frees == kSteps && g_bad_frees == 0 && g_live.size() == 1);
        h->own.release();
        CHECK(g_frees == kSteps);
        uint8_t *again = nullptr, *nothing = reinterpret_cast<uint8_t *>(1);
        CHECK(h->own.device_mem(&again, 32) == 0 && again && g_live.size() == 2);
        CHECK(h->own.device_mem(&nothing, 0) == 0 && nothing == nullptr);        // zero bytes: a null pointer, nothing recorded
        delete h;
        CHECK(g_frees == kSteps + 1 && g_bad_frees == 0 && g_live.size() == 1);
    }
    // ---- devices: frees happen with the owner's device current, the caller's is put back
    {
        reset_counters();
        g_cur = 0;
        Handle *h = new Handle(3);                                  // an owner on device 3 ...
        g_cur = 3;
        CHECK(build(h) == 0);
        g_cur = 0;                                                  // ... destroyed from a thread on device 0
        g_sets.clear();
        g_free_device = 3;
        delete h;
        CHECK(g_frees == kSteps && g_frees_off_device == 0 && g_bad_frees == 0);
        CHECK(g_cur == 0 && g_sets.size() == 2 && g_sets[0] == 3 && g_sets[1] == 0);
        // the same device: no device call at all
        reset_counters();
        g_cur = 5;
        h = new Handle(5);
        CHECK(build(h) == 0);
        g_free_device = 5;
        delete h;
        CHECK(g_frees == kSteps && g_frees_off_device == 0 && g_cur == 5 && g_sets.empty());
        // an empty owner: nothing to free, no device call
        reset_counters();
        g_cur = 1;
        delete new Handle(6);
        CHECK(g_frees == 0 && g_sets.empty() && g_cur == 1);
        // the owner's device cannot be made current: everything still goes back once (the runtime frees by pointer), and the
        // caller's device is left as it was - nothing to restore
        reset_counters();
        g_cur = 2;
        h = new Handle(4);
        CHECK(build(h) == 0);
        g_set_fails = true;
        g_sets.clear();
        delete h;
        g_set_fails = false;
        CHECK(g_frees == kSteps && g_bad_frees == 0 && g_cur == 2 && g_sets.size() == 1 && g_sets[0] == 4);
        // a create that fails half way on another device: the same holds for its partial set
        reset_counters();
        g_cur = 0;
        g_fail_at = 5;
        h = new Handle(7);
        CHECK(build(h) == kRefused);
        g_free_device = 7;
        delete h;
        CHECK(g_frees == 4 && g_frees_off_device == 0 && g_bad_frees == 0 && g_cur == 0);
    }
    CHECK(g_live.size() == 1);
    MockApi::device_free(bystander);
    CHECK(g_live.empty() && g_bad_frees == 0);
    printf("ok\n");
    return 0;
}
