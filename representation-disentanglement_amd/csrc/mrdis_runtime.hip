// mrdis_runtime.hip -- the host runtime of libmrdis_hip, no device code: the process-wide switches (mrdis_set_option / mrdis_get_option), the launch
// counters, the dynamic-LDS table behind MRDIS_LAUNCH, the per-kernel launch-setup caches (mrdis_common.h) and mrdis_strerror / mrdis_version.
#include "mrdis_common.h"
#include <mutex>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>

// ---------------------------------------------------------------------------------------------- process-wide switches
namespace {
struct OptDef { const char* name; const char* env; int is_flag; long long dflt; };
#define MRDIS_X_OPT_DEF(id, name, env, is_flag, dflt) {name, env, is_flag, dflt},
const OptDef OPT_DEFS[MRDIS_OPT_COUNT] = {MRDIS_OPTIONS(MRDIS_X_OPT_DEF)};        // what each switch means: at its line of MRDIS_OPTIONS (mrdis_common.h)
long long* opt_table() {
    static long long* table = [] {
        static long long v[MRDIS_OPT_COUNT];
        for (int i = 0; i < MRDIS_OPT_COUNT; ++i) {
            const char* e = getenv(OPT_DEFS[i].env);
            v[i] = !e ? OPT_DEFS[i].dflt : (OPT_DEFS[i].is_flag ? 1 : atoll(e));
        }
        return v;
    }();
    return table;
}
int opt_index(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < MRDIS_OPT_COUNT; ++i)
        if (!strcmp(name, OPT_DEFS[i].name)) return i;
    return -1;
}
}  // namespace
// relaxed atomics: launchers on any thread read the table while mrdis_set_option / mrdis_opt_note write it
long long mrdis_opt(int id) { return __atomic_load_n(&opt_table()[id], __ATOMIC_RELAXED); }
void mrdis_opt_note(int id, long long value) { __atomic_store_n(&opt_table()[id], value, __ATOMIC_RELAXED); }
extern "C" int mrdis_set_option(const char* name, long long value) {
    const int i = opt_index(name);
    if (i < 0) return MRDIS_EINVAL;
    mrdis_opt_note(i, value);
    return MRDIS_OK;
}
extern "C" long long mrdis_get_option(const char* name) {
    const int i = opt_index(name);
    return i < 0 ? (long long)MRDIS_EINVAL : mrdis_opt(i);
}

namespace {
#define MRDIS_X_CNT_NAME(id, name) name,
const char* const CNT_NAMES[MRDIS_CNT_COUNT] = {MRDIS_COUNTERS(MRDIS_X_CNT_NAME)};
long long g_counts[MRDIS_CNT_COUNT];
}  // namespace
void mrdis_count(int id) { __atomic_fetch_add(&g_counts[id], 1LL, __ATOMIC_RELAXED); }
extern "C" long long mrdis_launch_count(const char* family) {
    if (!family) return MRDIS_EINVAL;
    for (int i = 0; i < MRDIS_CNT_COUNT; ++i)
        if (!strcmp(family, CNT_NAMES[i])) return __atomic_load_n(&g_counts[i], __ATOMIC_RELAXED);
    return MRDIS_EINVAL;
}
extern "C" void mrdis_launch_count_reset(void) {
    for (int i = 0; i < MRDIS_CNT_COUNT; ++i) __atomic_store_n(&g_counts[i], 0LL, __ATOMIC_RELAXED);
}

namespace {
struct LdsNote { const char* expr; size_t bytes; };
LdsNote g_lds[128]; int g_nlds = 0;
std::mutex g_lds_mu;        // forward (main thread) and backward (autograd thread) both launch
}  // namespace
void mrdis_note_lds(const char* kernel_expr, size_t bytes) {       // host, launch path: a pointer compare per known kernel (string literals are unique per call site)
    const int n = __atomic_load_n(&g_nlds, __ATOMIC_ACQUIRE);
    for (int i = 0; i < n; ++i)        // known kernel at a size already seen: no lock (entries are only ever appended, bytes only ever grow)
        if (g_lds[i].expr == kernel_expr && bytes <= g_lds[i].bytes) return;
    std::lock_guard<std::mutex> lk(g_lds_mu);
    for (int i = 0; i < g_nlds; ++i)
        if (g_lds[i].expr == kernel_expr) { if (bytes > g_lds[i].bytes) g_lds[i].bytes = bytes; return; }
    if (g_nlds < 128) { g_lds[g_nlds].expr = kernel_expr; g_lds[g_nlds].bytes = bytes; __atomic_store_n(&g_nlds, g_nlds + 1, __ATOMIC_RELEASE); }
}
// "kernel expression=bytes" lines, at most cap - 1 characters, only whole lines; returns the number of entries written
extern "C" int mrdis_dynamic_lds_table(char* buf, int cap) {
    int pos = 0, written = 0;
    if (!buf || cap < 1) return MRDIS_EINVAL;
    buf[0] = 0;
    std::lock_guard<std::mutex> lk(g_lds_mu);
    for (int i = 0; i < g_nlds; ++i) {
        const int n = snprintf(buf + pos, (size_t)(cap - pos), "%s=%zu\n", g_lds[i].expr, g_lds[i].bytes);
        if (n < 0 || pos + n >= cap) { buf[pos] = 0; break; }      // the entry did not fit: drop its truncated text
        pos += n; ++written;
    }
    return written;
}

// ---------------------------------------------------------------------------------------------- launch setup (mrdis_common.h)
int mrdis_cu_count() {
    static const int ncu = [] {
        int dev = 0, n = 0;
        (void)hipGetDevice(&dev);
        return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
    }();
    return ncu;
}

namespace {
// Open-addressed tables keyed by kernel address.  Slots are only ever filled, under g_setup_mu, and a slot's key is stored last (release), so a
// reader that sees the key also sees the rest; an opt-in size only grows and is read atomically.
constexpr unsigned SETUP_SLOTS = 512;         // power of two, well above the kernels the library can launch
struct OptinSlot { const void* fn; int bytes; };
struct OccSlot { const void* fn; int block; size_t lds; int n; };
OptinSlot g_optin[SETUP_SLOTS];
OccSlot g_occ[SETUP_SLOTS];
std::mutex g_setup_mu;
unsigned setup_hash(const void* fn) { return (unsigned)(((uintptr_t)fn * 0x9E3779B97F4A7C15ull) >> 40); }
}  // namespace

bool mrdis_lds_optin(const void* kernel, int bytes) {
    const unsigned h = setup_hash(kernel);
    for (unsigned i = 0; i < SETUP_SLOTS; ++i) {
        OptinSlot& e = g_optin[(h + i) % SETUP_SLOTS];
        const void* fn = __atomic_load_n(&e.fn, __ATOMIC_ACQUIRE);
        if (fn == kernel && __atomic_load_n(&e.bytes, __ATOMIC_RELAXED) >= bytes) return true;
        if (!fn || fn == kernel) break;
    }
    std::lock_guard<std::mutex> lk(g_setup_mu);
    OptinSlot* slot = nullptr;             // this kernel's slot or the first free one; none when the table is full (then nothing is cached)
    for (unsigned i = 0; i < SETUP_SLOTS && !slot; ++i) {
        OptinSlot& e = g_optin[(h + i) % SETUP_SLOTS];
        if (!e.fn || e.fn == kernel) slot = &e;
    }
    if (slot && slot->fn == kernel && slot->bytes >= bytes) return true;       // another thread opted it in meanwhile
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    if (slot) { __atomic_store_n(&slot->bytes, bytes, __ATOMIC_RELAXED); __atomic_store_n(&slot->fn, kernel, __ATOMIC_RELEASE); }
    return true;
}

int mrdis_occupancy(const void* kernel, int block, size_t lds) {
    const unsigned h = setup_hash(kernel);
    for (unsigned i = 0; i < SETUP_SLOTS; ++i) {
        const OccSlot& e = g_occ[(h + i) % SETUP_SLOTS];
        const void* fn = __atomic_load_n(&e.fn, __ATOMIC_ACQUIRE);
        if (!fn) break;
        if (fn == kernel && e.block == block && e.lds == lds) return e.n;
    }
    std::lock_guard<std::mutex> lk(g_setup_mu);
    OccSlot* slot = nullptr;
    for (unsigned i = 0; i < SETUP_SLOTS && !slot; ++i) {
        OccSlot& e = g_occ[(h + i) % SETUP_SLOTS];
        if (!e.fn || (e.fn == kernel && e.block == block && e.lds == lds)) slot = &e;
    }
    if (slot && slot->fn) return slot->n;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, lds) != hipSuccess || n < 1) return 0;
    if (slot) { slot->block = block; slot->lds = lds; slot->n = n; __atomic_store_n(&slot->fn, kernel, __ATOMIC_RELEASE); }
    return n;
}

extern "C" const char* mrdis_strerror(int code) {
    switch (code) {
        case MRDIS_OK: return "ok";
        case MRDIS_EINVAL: return "invalid argument";
        case MRDIS_EUNSUPPORTED: return "unsupported geometry";
        case MRDIS_EWORKSPACE: return "workspace too small";
        case MRDIS_ELAUNCH: return "kernel launch failed";
        case MRDIS_EALIGN: return "misaligned pointer or leading dimension";
        default: return "unknown error";
    }
}
extern "C" int mrdis_version(void) { return 110; }
