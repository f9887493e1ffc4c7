// Episode bookkeeping on the device (include/procgen2_vec.h pgv_step_episodes): which envs ended in this step, what their
// episodes scored and how long they took, their terminal frames — decided behind the step's render launch, on the env's
// stream, so that a same-step auto-reset needs no look from the host.
//
// Three small launches a step, ordered by the stream and by nothing else (no flags, no spinning, no look-back):
//   * episode_before_kernel, in front of the step: the `done` row as the step finds it.  An env whose row is set has its
//     reset served by this step (reward 0, done 0, the reset frame): not an episode step.  Read from the row itself, so it
//     holds after pgv_load_envs / pgv_load_state and between calls of pgv_step.
//   * episode_rule_kernel, behind the step: a lane per env applies episode_step() below to the env's running counters,
//     writes the per-env outputs, keeps an ended env's return and length, and leaves its workgroup's count of ended envs.
//   * episode_list_kernel: a workgroup's base in the ascending list is the sum of the counts of the workgroups in front of
//     it (at most n / 256 words, 256 at 65 536 envs), a lane's place inside it a wave ballot plus the wave prefix in LDS.
//     Then the workgroup copies the frames of its own ended envs whose place lies below the ring's capacity: 12 288 bytes a
//     frame, 768 16-byte vectors over 256 lanes.  A step in which every env ends still moves capacity × 12 KB and no more.
// Bounds: every list index is below the number of ended envs <= n; a ring row is written only where place < capacity.
#pragma once

#include "pg_carve.h"
#include "pg_defs.h"

namespace pg {

constexpr int kEpisodeBlock = 256;  // envs a workgroup (both kernels: the counts of one are the bases of the other)
constexpr int kEpisodeWaves = kEpisodeBlock / 64;
static_assert(kEpisodeBlock % 64 == 0, "whole wavefronts");

// The per-env rule.  `prev_done`: the env's `done` row as the step found it (non-zero: this step served its reset).
// A counted step adds its reward to the return — one float32 addition a step, in step order — and one to the length.  An
// episode ends when the game says so (terminated), or, with a limit, when it has played its max_steps-th step without
// that (truncated).  >= and not ==: a caller may write the running length (after a fork), and a value already past the
// limit must not run for ever.
struct EpisodeStep {
    float ret;
    int32_t len;
    uint8_t counted, terminated, truncated, ended;
};
PG_HD EpisodeStep episode_step(float ret, int32_t len, float reward, uint8_t done, uint8_t prev_done, int32_t max_steps) {
    EpisodeStep s;
    s.counted = prev_done == 0;
    s.terminated = done != 0;
    s.truncated = 0;
    if (s.counted) {
        ret = ret + reward;
        len = len + 1;
        s.truncated = !s.terminated && max_steps > 0 && len >= max_steps;
    }
    s.ret = ret;
    s.len = len;
    s.ended = s.terminated | s.truncated;
    return s;
}

// A lane's place among the set lanes of its wave's ballot, and a wave's share of the list.
PG_HD int episode_rank_in_wave(uint64_t ballot, int lane) {
    return __builtin_popcountll(ballot & ((uint64_t(1) << lane) - uint64_t(1)));
}
PG_HD int episode_frames_of_block(int base, int count, int capacity) {  // how many of a workgroup's ended envs get a ring row
    const int room = capacity - base;
    return room <= 0 ? 0 : (count < room ? count : room);
}

struct EpisodeBuffers {
    int n, max_steps, capacity;
    // inputs: the engine's rows (StepIO) and level words (LevelPlan)
    const uint8_t* obs;
    const float* step_reward;
    const uint8_t* done;
    const uint32_t* level_number;
    const uint8_t* level_known;
    // outputs (pgv_episode_outputs)
    float* reward;
    uint8_t *terminated, *truncated, *ended;
    int32_t* counts;
    int32_t* ended_env;
    float* ended_return;
    int32_t* ended_length;
    uint32_t* ended_level;
    uint8_t* ended_level_known;
    uint8_t* final_obs;
    float* running_return;
    int32_t* running_length;
    // between the kernels
    uint8_t* prev_done;      // [n]
    float* kept_return;      // [n]  of the episode that ended in this step
    int32_t* kept_length;    // [n]
    int32_t* block_count;    // [ceil(n / 256)]
};
inline int episode_blocks(int n) { return (n + kEpisodeBlock - 1) / kEpisodeBlock; }
// The one device block behind the seventeen buffers (pg_carve.h): n and b.capacity say how big they are.
inline void list_episodes(Carve& c, EpisodeBuffers& b, int n) {
    const size_t envs = size_t(n);
    c.take(b.reward, envs * 4);
    c.take(b.terminated, envs);
    c.take(b.truncated, envs);
    c.take(b.ended, envs);
    c.take(b.counts, 8);  // [0] ended envs, [1] ring rows written
    c.take(b.ended_env, envs * 4);
    c.take(b.ended_return, envs * 4);
    c.take(b.ended_length, envs * 4);
    c.take(b.ended_level, envs * 4);
    c.take(b.ended_level_known, envs);
    c.take(b.running_return, envs * 4);
    c.take(b.running_length, envs * 4);
    c.take(b.prev_done, envs);
    c.take(b.kept_return, envs * 4);
    c.take(b.kept_length, envs * 4);
    c.take(b.block_count, size_t(episode_blocks(n)) * 4);
    c.take(b.final_obs, size_t(b.capacity) * kObsBytes);  // (no ring: nullptr)
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(kEpisodeBlock) episode_before_kernel(EpisodeBuffers b) {
    const int i = static_cast<int>(blockIdx.x) * kEpisodeBlock + static_cast<int>(threadIdx.x);
    if (i < b.n) b.prev_done[i] = b.done[i];
}

// pgv_reset on an engine that keeps episodes: the envs it names start their episodes afresh.
__global__ void __launch_bounds__(kEpisodeBlock) episode_clear_kernel(EpisodeBuffers b, const uint8_t* mask) {
    const int i = static_cast<int>(blockIdx.x) * kEpisodeBlock + static_cast<int>(threadIdx.x);
    if (i >= b.n || (mask && !mask[i])) return;
    b.running_return[i] = 0.0f;
    b.running_length[i] = 0;
}

__global__ void __launch_bounds__(kEpisodeBlock) episode_rule_kernel(EpisodeBuffers b) {
    __shared__ int wave_count[kEpisodeWaves];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int i = static_cast<int>(blockIdx.x) * kEpisodeBlock + tid;
    bool ended = false;
    if (i < b.n) {
        const float r = b.step_reward[i];
        const EpisodeStep s = episode_step(b.running_return[i], b.running_length[i], r, b.done[i], b.prev_done[i], b.max_steps);
        ended = s.ended != 0;
        b.reward[i] = r;
        b.terminated[i] = s.terminated;
        b.truncated[i] = s.truncated;
        b.ended[i] = s.ended;
        if (ended) {
            b.kept_return[i] = s.ret;
            b.kept_length[i] = s.len;
        }
        b.running_return[i] = ended ? 0.0f : s.ret;
        b.running_length[i] = ended ? 0 : s.len;
    }
    const uint64_t ballot = __ballot(ended);  // (wave64: one bit a lane; lanes past n vote 0)
    if (lane == 0) wave_count[wave] = __builtin_popcountll(ballot);
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int w = 0; w < kEpisodeWaves; w++) sum += wave_count[w];
        b.block_count[blockIdx.x] = sum;
    }
}

__global__ void __launch_bounds__(kEpisodeBlock) episode_list_kernel(EpisodeBuffers b) {
    __shared__ int wave_sum[kEpisodeWaves], wave_all[kEpisodeWaves], wave_count[kEpisodeWaves];
    __shared__ int32_t frame_env[kEpisodeBlock];  // the workgroup's ended envs, by their place in it
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int block = static_cast<int>(blockIdx.x), blocks = static_cast<int>(gridDim.x);
    const int i = block * kEpisodeBlock + tid;
    // the base: the counts of the workgroups in front (workgroup 0 also adds up all of them, for counts[])
    int before = 0, all = 0;
    const int upto = block == 0 ? blocks : block;
    for (int k = tid; k < upto; k += kEpisodeBlock) {
        const int c = b.block_count[k];
        all += c;
        if (k < block) before += c;
    }
    for (int d = 32; d > 0; d >>= 1) {
        before += __shfl_xor(before, d, 64);
        all += __shfl_xor(all, d, 64);
    }
    const bool ended = i < b.n && b.ended[i] != 0;
    const uint64_t ballot = __ballot(ended);
    if (lane == 0) {
        wave_sum[wave] = before;
        wave_all[wave] = all;
        wave_count[wave] = __builtin_popcountll(ballot);
    }
    __syncthreads();
    int base = 0, total = 0, here = 0;
    for (int w = 0; w < kEpisodeWaves; w++) base += wave_sum[w], total += wave_all[w], here += wave_count[w];
    if (block == 0 && tid == 0) {
        b.counts[0] = total;
        b.counts[1] = total < b.capacity ? total : b.capacity;
    }
    int place = episode_rank_in_wave(ballot, lane);  // in the workgroup
    for (int w = 0; w < wave; w++) place += wave_count[w];
    if (ended) {
        const int k = base + place;  // < the number of ended envs <= n
        b.ended_env[k] = i;
        b.ended_return[k] = b.kept_return[i];
        b.ended_length[k] = b.kept_length[i];
        b.ended_level[k] = b.level_number[i];
        b.ended_level_known[k] = b.level_known[i];
        frame_env[place] = i;
    }
    __syncthreads();
    const int frames = episode_frames_of_block(base, here, b.capacity);  // rows base .. base + frames - 1 < capacity
    for (int f = 0; f < frames; f++) {
        const uint4* from = reinterpret_cast<const uint4*>(b.obs + size_t(frame_env[f]) * kObsBytes);
        uint4* to = reinterpret_cast<uint4*>(b.final_obs + size_t(base + f) * kObsBytes);
        for (int v = tid; v < kObsBytes / 16; v += kEpisodeBlock) to[v] = from[v];
    }
}

inline void launch_episode_before(hipStream_t st, const EpisodeBuffers& b) {
    hipLaunchKernelGGL(episode_before_kernel, dim3(episode_blocks(b.n)), dim3(kEpisodeBlock), 0, st, b);
}
inline void launch_episode_clear(hipStream_t st, const EpisodeBuffers& b, const uint8_t* mask) {
    hipLaunchKernelGGL(episode_clear_kernel, dim3(episode_blocks(b.n)), dim3(kEpisodeBlock), 0, st, b, mask);
}
inline void launch_episode_after(hipStream_t st, const EpisodeBuffers& b) {
    hipLaunchKernelGGL(episode_rule_kernel, dim3(episode_blocks(b.n)), dim3(kEpisodeBlock), 0, st, b);
    hipLaunchKernelGGL(episode_list_kernel, dim3(episode_blocks(b.n)), dim3(kEpisodeBlock), 0, st, b);
}
#endif

}  // namespace pg
