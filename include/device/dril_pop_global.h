// dril_pop_global.h — the ONE definition of pop_global: what a population kernel does with a pointer it read out of a member's argument block.  Device code only
// (hipcc); the library's population kernels (dril_pop_map.h) and a plug-in's own (device/dril_env_rollout_pop.h) both take it from here.
#pragma once

#if defined(__HIPCC__)
namespace dril {
// A pointer read out of a member's argument block is a generic pointer to the compiler, and every access through it a flat one; a kernel argument is known to be
// global.  The round trip through the global address space gives the block's pointers that knowledge back (null stays null), so a member's loop issues the same
// global loads, stores and atomics as its solo twin.  The empty asm keeps the optimiser from folding the two casts away; the pointers are uniform (scalar registers).
template <class T> __device__ __forceinline__ T* pop_global(T* p) {
    auto g = (__attribute__((address_space(1))) T*)p;
    asm("" : "+s"(g));
    return (T*)g;
}
// Member m's block of a table of argument blocks, read IN PLACE through the constant address space: every field is a uniform (scalar) load where it is used, an array
// inside the block may be indexed at run time without a private copy (which would live in scratch memory), and a pointer loaded from constant memory is a global
// pointer to the compiler — the round trip of pop_global, for a whole block at once.  The table must not be written while the kernel runs (the host fills it before
// the launch, in stream order).  The cast comes BEFORE the indexing, so that every load's address is a constant-address-space pointer from the start.
template <class T> __device__ __forceinline__ const T& pop_member_block(const T* table, unsigned m) {
    return *(const T*)((const __attribute__((address_space(4))) T*)table + m);
}
}  // namespace dril
#endif
