// The device side of a batch stop (kSticky*, StopStage: bsa_internal.h), shared by the stopping
// stages' launches (k_sim_cond, k_sim_exparea).  word = {sticky (low 32 bits), stop_word(stage, tag) (high)}, read
// and raised as one 64-bit word, so every wave of a raising launch sees its own step's tag.
#pragma once
#include "bsa_wave.h"

namespace bsa {

// Does this launch of the batch's step `tag` still run?  Behind the sticky word like every stage -- except behind
// a stop that carries this very step's tag, whichever stage raised it: an earlier stopping launch of the step or
// another wave of this one.  The stopping step is complete, so each of its stopping launches runs in full.  (An
// abort carries tag 0, tags start at 1; a stop of an earlier step carries an earlier tag.)  One read per wave
__device__ __forceinline__ bool stop_runs(const unsigned long long *word, unsigned tag) {
  const unsigned long long w = wave_bcast_u64(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  return (unsigned)w == 0u || stop_tag((unsigned)(w >> 32)) == tag;
}

// One lane of a wave with something for the host: the stage's pending word takes the step's tag (every writer of
// a launch stores the same value), and the stop is raised only while the word is 0 (vector atomics)
__device__ __forceinline__ void stop_raise(unsigned long long *word, unsigned long long *pend, StopStage stage,
                                           unsigned tag) {
  __hip_atomic_store(pend + stage, (unsigned long long)tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicCAS(word, 0ull, ((unsigned long long)stop_word(stage, tag) << 32) | (unsigned long long)kStickyStopped);
}

}  // namespace bsa
