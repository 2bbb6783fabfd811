"""CPU: the owners of device and pinned memory (dril.jl_amd/csrc/dril_devmem.h), without a GPU.  The header leaves its four allocation functions to a host
compile; the driver below defines them over malloc / free with a log of every pointer handed out and taken back, keeps the live-bytes count as the library's own
definitions do, and refuses an allocation above 1 MiB.  It is a stand-alone program (g++ -fsanitize=address,undefined), run as a child process: the first violated
claim prints its line and exits non-zero; every claim is re-checked against the log after every step."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

_DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#include "dril_devmem.h"
using namespace dril;

namespace {
struct Entry { size_t bytes; bool pinned; int frees; };
std::map<void*, Entry> g_log;                      // every pointer ever handed out (never reused: a freed block is kept until exit)
std::vector<void*> g_kept;
int g_allocs = 0, g_frees = 0;
constexpr size_t kRefuseAbove = 1 << 20;
int fake_alloc(void** p, size_t bytes, bool pinned, bool zero) {
    if (bytes > kRefuseAbove) return 2;            // "out of memory"
    char* q = (char*)std::malloc(bytes);
    for (size_t i = 0; i < bytes; ++i) q[i] = zero ? 0 : 0x5a;
    g_log[q] = Entry{bytes, pinned, 0}; g_allocs += 1;
    *p = q; g_devmem_live_bytes += (int64_t)bytes;
    return 0;
}
void fake_free(void* p, size_t bytes, bool pinned) {
    auto it = g_log.find(p);
    if (it == g_log.end()) { std::printf("free of a pointer never handed out\n"); std::exit(3); }
    if (it->second.bytes != bytes || it->second.pinned != pinned) { std::printf("free with another size or kind than the allocation\n"); std::exit(3); }
    it->second.frees += 1; g_frees += 1; g_kept.push_back(p);   // the block itself goes at exit, so that no address comes back
    g_devmem_live_bytes -= (int64_t)bytes;
}
}  // namespace
namespace dril {
devmem_err_t devmem_alloc_device(void** p, size_t bytes, bool zero) { return fake_alloc(p, bytes, false, zero); }
void devmem_free_device(void* p, size_t bytes) { fake_free(p, bytes, false); }
devmem_err_t devmem_alloc_pinned(void** p, size_t bytes) { return fake_alloc(p, bytes, true, false); }
void devmem_free_pinned(void* p, size_t bytes) { fake_free(p, bytes, true); }
}  // namespace dril

namespace {
int frees_of(void* p) { return g_log.at(p).frees; }
// after every step: nothing freed twice, and the count is the sum of what is held (the caller states that sum)
void settle(int line, int64_t held_bytes) {
    int64_t live = 0;
    for (auto& kv : g_log) {
        if (kv.second.frees > 1) { std::printf("line %d: a pointer was freed %d times\n", line, kv.second.frees); std::exit(1); }
        if (kv.second.frees == 0) live += (int64_t)kv.second.bytes;
    }
    if (live != held_bytes || g_devmem_live_bytes.load() != held_bytes) {
        std::printf("line %d: live bytes: log %lld, counter %lld, owners hold %lld\n", line, (long long)live, (long long)g_devmem_live_bytes.load(), (long long)held_bytes); std::exit(1);
    }
}
#define CLAIM(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
#define SETTLE(bytes) settle(__LINE__, (int64_t)(bytes))

template <typename T> T* as_ptr(T* p) { return p; }   // what a use site does: the owner converts

template <class Buf, typename T> void exercise(bool pinned) {
    SETTLE(0);
    {   // alloc(0): a non-null buffer of one element
        Buf b; CLAIM(!b && b.get() == nullptr && b.size() == 0);
        CLAIM(b.alloc(0) == 0 && b.get() != nullptr && b.size() == 1); SETTLE(sizeof(T));
        CLAIM(g_log.at(b.get()).pinned == pinned);
    }   // scope exit frees
    SETTLE(0);
    {   // alloc on a held buffer frees the old pointer exactly once
        Buf b; CLAIM(b.alloc(5) == 0); T* p0 = b; SETTLE(5 * sizeof(T));
        CLAIM(b.alloc(9) == 0 && b.get() != p0 && b.size() == 9 && frees_of(p0) == 1); SETTLE(9 * sizeof(T));
        CLAIM(as_ptr<T>(b) == b.get() && &b[2] == b.get() + 2 && b + 1 == b.get() + 1);           // the forms a use site relies on
    }
    SETTLE(0);
    {   // grow: n <= size keeps pointer and size and reports false; n > size frees once, reports true, size n
        Buf b; bool grew = false;
        CLAIM(b.grow(4, &grew) == 0 && grew && b.size() == 4); T* p0 = b; SETTLE(4 * sizeof(T));
        CLAIM(b.grow(4, &grew) == 0 && !grew && b.get() == p0 && b.size() == 4); SETTLE(4 * sizeof(T));
        CLAIM(b.grow(1, &grew) == 0 && !grew && b.get() == p0 && b.size() == 4 && frees_of(p0) == 0); SETTLE(4 * sizeof(T));
        CLAIM(b.grow(7, &grew) == 0 && grew && b.get() != p0 && b.size() == 7 && frees_of(p0) == 1); SETTLE(7 * sizeof(T));
        CLAIM(b.grow(6) == 0 && b.size() == 7);                                                     // the report is optional
        T* p1 = b; CLAIM(b.grow_zero(8, &grew) == 0 && grew && b.size() == 8 && frees_of(p1) == 1); SETTLE(8 * sizeof(T));
    }
    SETTLE(0);
    {   // move construction and move assignment leave the source empty and free nothing twice
        Buf a; CLAIM(a.alloc(3) == 0); T* pa = a;
        Buf b(std::move(a)); CLAIM(!a && a.size() == 0 && b.get() == pa && b.size() == 3 && frees_of(pa) == 0); SETTLE(3 * sizeof(T));
        Buf c; CLAIM(c.alloc(2) == 0); T* pc = c; SETTLE(5 * sizeof(T));
        c = std::move(b); CLAIM(!b && b.size() == 0 && c.get() == pa && c.size() == 3 && frees_of(pc) == 1 && frees_of(pa) == 0); SETTLE(3 * sizeof(T));
        Buf& self = c; c = std::move(self); CLAIM(c.get() == pa && c.size() == 3 && frees_of(pa) == 0); SETTLE(3 * sizeof(T));   // onto itself: nothing happens
        // std::swap of two owners frees nothing
        Buf d; CLAIM(d.alloc(6) == 0); T* pd = d; const int before = g_frees;
        std::swap(c, d); CLAIM(c.get() == pd && c.size() == 6 && d.get() == pa && d.size() == 3 && g_frees == before); SETTLE(9 * sizeof(T));
        Buf e; std::swap(d, e); CLAIM(!d && e.get() == pa && g_frees == before); SETTLE(9 * sizeof(T));                          // with an empty one too
        // release() twice frees once
        c.release(); CLAIM(!c && c.size() == 0 && frees_of(pd) == 1); SETTLE(3 * sizeof(T));
        c.release(); CLAIM(frees_of(pd) == 1 && g_frees == before + 1); SETTLE(3 * sizeof(T));
    }
    SETTLE(0);
    {   // a failing allocation leaves the owner empty and the count unchanged: on an empty owner, on a held one (its buffer is gone: alloc frees first), through grow
        Buf b; CLAIM(b.alloc(kRefuseAbove / sizeof(T) + 1) != 0 && !b && b.size() == 0); SETTLE(0);
        CLAIM(b.alloc(2) == 0); T* p0 = b; SETTLE(2 * sizeof(T));
        CLAIM(b.alloc(kRefuseAbove / sizeof(T) + 1) != 0 && !b && b.size() == 0 && frees_of(p0) == 1); SETTLE(0);
        bool grew = false; CLAIM(b.grow(kRefuseAbove / sizeof(T) + 1, &grew) != 0 && grew && !b); SETTLE(0);
        CLAIM(b.alloc(kRefuseAbove / sizeof(T)) == 0 && b.size() == kRefuseAbove / sizeof(T)); SETTLE(kRefuseAbove);               // the largest that fits still does
    }
    SETTLE(0);
}
}  // namespace

int main() {
    exercise<DevBuf<float>, float>(false);
    exercise<PinnedBuf<double>, double>(true);
    exercise<DevBuf<char>, char>(false);
    {   // alloc_zero asks the device for cleared memory; alloc does not (the fake fills 0x5a)
        DevBuf<int> z; CLAIM(z.alloc_zero(16) == 0); for (int i = 0; i < 16; ++i) CLAIM(z[i] == 0);
        CLAIM(z.alloc(16) == 0 && z[0] == 0x5a5a5a5a);
        CLAIM(z.alloc_zero(0) == 0 && z.size() == 1 && z[0] == 0);
    }
    {   // owners as members and in a vector: what a handle does
        struct Handle { DevBuf<float> a, b; PinnedBuf<int> c; std::vector<PinnedBuf<char>> blocks; };
        Handle* h = new Handle; CLAIM(h->a.alloc(10) == 0 && h->c.alloc(1) == 0);
        h->blocks.resize(3); for (auto& blk : h->blocks) CLAIM(blk.alloc(100) == 0);
        h->blocks.resize(17);                                                                       // reallocation of the vector moves the owners: nothing is freed
        CLAIM(g_devmem_live_bytes.load() == 40 + 4 + 300);
        const float* alias = h->b ? h->b : h->a; CLAIM(alias == h->a.get());                         // `c ? owner : owner`, `if (!owner)`
        delete h;
    }
    settle(__LINE__, 0);                                                                            // the live count is 0 at exit
    for (auto& kv : g_log) if (kv.second.frees != 1) { std::printf("a pointer was freed %d times\n", kv.second.frees); return 1; }   // every pointer exactly once
    if (g_allocs != g_frees || g_allocs != (int)g_log.size()) { std::printf("allocs %d frees %d log %zu\n", g_allocs, g_frees, g_log.size()); return 1; }
    for (void* p : g_kept) std::free(p);
    std::printf("devmem ok: %d allocations, each freed once\n", g_allocs);
    return 0;
}
'''


def test_owners_free_each_pointer_once_and_keep_the_count(tmp_path):
    src = tmp_path / "devmem_check.cpp"; src.write_text(_DRIVER)
    exe = tmp_path / "devmem_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", str(ROOT / "dril.jl_amd" / "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("devmem ok:"), r.stdout
