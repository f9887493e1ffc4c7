"""ProcgenVecEnv — N concurrent envs on one MI355X, tensors stay in HBM.

Counterpart of the reference's `CEnv` (cenv/cenv.py:152-380) for the vector extension
(include/procgen2_vec.h): same life cycle (make → reset → step … close), but observations,
rewards and dones are zero-copy torch tensors over the engine's output slab instead of per-call
numpy copies (SURVEY.md §8b "Consequence for a vector engine").

Multi-GPU: one process per GPU; rank r owns global envs [r*N, (r+1)*N) (seed = seed_base + global
index, so results do not depend on the GPU count).  There is no collective in reset/step/render;
`gather()` is the optional rooted gather of obs/reward/done to rank 0 over RCCL.
"""
import collections
import ctypes
import os
from ctypes import c_void_p

import torch

from . import lib as pglib

GAMES = ("coinrun", "maze", "bossfight", "climber", "caveflyer", "chaser", "jumper")
_SEQUENCES_KEPT = 4  # ProcgenVecEnv.step_sequence: result sets kept, by T


def shard_range(total_envs, world_size, rank):
    """Contiguous env-index block of `rank`: [lo, hi).  Earlier ranks take the remainder."""
    base, rem = divmod(total_envs, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class ProcgenVecEnv:
    def __init__(self, game, num_envs, device=0, seed_base=1, env_offset=0, lib_path=None, num_levels=0,
                 start_level=0, distribution_mode=None, game_flags=0, out=None, autoreset_mode=None, max_episode_steps=0,
                 final_obs_capacity=0, policy_obs=None, history=None, transitions=False):
        """transitions = False | True (needs history=): the record ring beside the frame history (include/procgen2_vec.h
        pgv_transitions_enable) — `transitions`, a TransitionTensors: zero-copy [T, N] views `action` int32, `reward` float32,
        `flags` u8 (pglib.TR_* bits); row q describes the call that made push q + 1.  transition_gather() for n-step
        transitions of any (push, env) pairs, transition_gae() for advantages over a stretch of the ring.  False changes nothing
        at all.

        history = None | dict(capacity=T, gray=False): frame history on the device (include/procgen2_vec.h
        pgv_history_enable) — `history`, a HistoryTensors: `frames` u8 [T, N, C, 64, 64] (C = 1 gray, 3 RGB), one frame per env
        and push in slot push % T, `began` u8 [T, N], `pending` u8 [N], `head` (the pushes so far) and `capacity`; every step,
        step_episodes and drawn sequence pushes a slot, reset() rewrites the newest; history_push() by hand and
        history_gather() for stacked, scaled rows of any (push, env) pairs.  None changes nothing at all.

        policy_obs = None | dict(stack=4, gray=True, dtype="float16"): policy-ready observations on the device
        (include/procgen2_vec.h pgv_policy_obs_enable) — `policy_obs`, a [N, K*C, 64, 64] tensor of that dtype ("uint8",
        "float16", "bfloat16", "float32"; C = 1 gray, 3 RGB; slot 0 the oldest frame) that every step, reset and drawn
        sequence keeps current, stacks restarted where an episode began; `policy_restart`, the pending restart flags;
        push_policy_obs() by hand.  Every return value stays as it is: the tensor is read from the attribute.  None changes
        nothing at all.

        autoreset_mode = None | "next_step" | "same_step": episodes on the device (include/procgen2_vec.h
        pgv_episodes_enable) — step_episodes() and the `episode` tensors; None changes nothing at all.  max_episode_steps
        (0: no limit; same_step only) truncates, final_obs_capacity (0 .. num_envs) is the rows of the terminal-frame ring.

        out = (obs, reward, done): caller-owned result tensors on `device` — uint8 [N,64,64,3], float32 [N],
        uint8 [N], contiguous — e.g. slices of one slab that several envs (the games of a mixed workload) fill side by
        side ("one contiguous [N_local,64,64,3] slab regardless of game").  Default: own tensors."""
        if not torch.cuda.is_available():
            raise pglib.EngineError("ProcgenVecEnv needs a HIP device (torch.cuda.is_available() is False); "
                                    "there is no CPU fallback")
        self.L = pglib.load(lib_path)
        self.game = game
        self.num_envs = int(num_envs)
        self.env_offset = int(env_offset)
        policy = _policy_obs_config(policy_obs)  # (ValueError before anything is made)
        ring = _history_config(history)
        if transitions not in (False, True):
            raise ValueError("transitions must be True or False")
        if transitions and ring is None:
            raise ValueError("transitions=True needs history=dict(capacity=T, ...) with T >= 2")
        if transitions and ring[0] < 2:
            raise ValueError("transitions=True needs a history capacity >= 2")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        # The engine gets a stream of its own (a torch stream, so torch can order against it): torch's default stream
        # has handle 0, which the C ABI reads as "create one", and work on an unrelated stream would race with the
        # caller's.  Every call below makes the engine's stream wait for the caller's current stream (actions, masks)
        # and the caller's current stream wait for the engine's (obs, reward, done).
        # (PG_STREAM_PRIORITY_<GAME>=-1: a high-priority stream for that game's engine — an A/B switch for several engines on
        # one GPU, bench.py --workload mixed; default 0)
        self._stream = torch.cuda.Stream(device=self.device, priority=int(os.environ.get("PG_STREAM_PRIORITY_" + game.upper(), "0")))
        # num_levels > 0: a finite level set (include/procgen2_vec.h pgv_make_levels); 0 = every level is new.
        # distribution_mode: None / "default" = the reference's compile-time config, or "easy" | "hard" | "memory" |
        # "extreme" where the game has it (pgv_game_modes).
        h = pglib.make(self.L, game, self.num_envs, device=device, seed_base=seed_base, env_offset=self.env_offset,
                       stream=c_void_p(self._stream.cuda_stream), num_levels=num_levels, start_level=start_level,
                       mode=distribution_mode, game_flags=game_flags)
        self.num_levels, self.start_level = int(num_levels), int(start_level)
        self.distribution_mode = {v: k for k, v in pglib.MODES.items()}[self.L.pgv_mode(h)]
        self._h = h
        # The columns of state_obs() / tile_obs() (include/procgen2_vec.h pgv_state_layout_of, pgv_state_names): width, fixed,
        # record, max_records, cells, tile_w, tile_h, fixed_names, record_names.
        self.state_layout = pglib.state_layout(self.L, game, self.distribution_mode)
        # What tile_paths() goes by (include/procgen2_vec.h pgv_path_layout_of): cells, tile_w, tile_h, has_goal, agent_dx, agent_dy.
        self.path_layout = pglib.path_layout(self.L, game, self.distribution_mode)
        # What get_levels() / set_levels() go by (include/procgen2_vec.h pgv_level_layout_of): supported, cells, tile_w, tile_h, backgrounds.
        self.level_layout = pglib.level_layout(self.L, game, self.distribution_mode)
        self._sequences = {}  # step_sequence's result tensors, by T: the _SEQUENCES_KEPT most recently used
        # torch owns the result buffers; the engine writes straight into them.
        if out is not None:
            self.obs, self.reward, self.done = out
            want = (((self.num_envs, 64, 64, 3), torch.uint8), ((self.num_envs,), torch.float32),
                    ((self.num_envs,), torch.uint8))
            for t, (shape, dtype) in zip(out, want):
                if tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                    self.L.pgv_close(h)
                    self._h = None
                    raise ValueError("out: expected a contiguous %s tensor of shape %s on %s" % (dtype, shape, self.device))
        else:
            self.obs = torch.zeros((self.num_envs, 64, 64, 3), dtype=torch.uint8, device=self.device)
            self.reward = torch.zeros(self.num_envs, dtype=torch.float32, device=self.device)
            self.done = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
        pglib.check(self.L, self.L.pgv_bind_outputs(self._h, c_void_p(self.obs.data_ptr()),
                                                    c_void_p(self.reward.data_ptr()), c_void_p(self.done.data_ptr())),
                    "pgv_bind_outputs")
        # The engine's own per-env level words (pgv_level_numbers / pgv_level_known), exposed the way obs is: zero-copy
        # tensors over device memory the engine writes in the step that installs a level.
        self.level_numbers = _device_view(self.L.pgv_level_numbers(h), self.num_envs, "<u4", self.device)
        self.level_known = _device_view(self.L.pgv_level_known(h), self.num_envs, "|u1", self.device)
        self.single_observation_shape = (64, 64, 3)
        self.num_actions = pglib.NUM_ACTIONS
        self.autoreset_mode, self.episode = autoreset_mode, None
        if autoreset_mode is None:
            if max_episode_steps or final_obs_capacity:
                self.close()
                raise ValueError("max_episode_steps / final_obs_capacity need autoreset_mode='next_step' or 'same_step'")
        else:
            try:
                if autoreset_mode not in pglib.AUTORESET_MODES:
                    raise ValueError("autoreset_mode must be None, 'next_step' or 'same_step'")
                self.episode = EpisodeTensors(pglib.episodes_enable(self.L, h, autoreset_mode, max_episode_steps, final_obs_capacity),
                                              self.num_envs, int(final_obs_capacity), self.device)
            except Exception:
                self.close()
                raise
        self.policy_obs = self.policy_restart = None
        if policy is not None:
            # torch owns the tensor, as it owns obs; the engine writes straight into it.
            stack, gray, dtype = policy
            self.policy_obs = torch.zeros((self.num_envs, stack * (1 if gray else 3), 64, 64), dtype=getattr(torch, dtype), device=self.device)
            try:
                self._before()
                pglib.policy_obs_enable(self.L, h, stack, gray, dtype, c_void_p(self.policy_obs.data_ptr()))
                self._after()
                self.policy_restart = _device_view(self.L.pgv_policy_obs_restart(h), self.num_envs, "|u1", self.device)
            except Exception:
                self.close()
                raise

        self.history = None
        if ring is not None:
            # torch owns the ring, as it owns obs; the engine writes straight into it.
            capacity, gray = ring
            try:
                frames = torch.zeros((capacity, self.num_envs, 1 if gray else 3, 64, 64), dtype=torch.uint8, device=self.device)
                self._before()
                pglib.history_enable(self.L, h, capacity, gray, c_void_p(frames.data_ptr()))
                self._after()
                self.history = HistoryTensors(self, frames)
            except Exception:
                self.close()
                raise
        self.transitions = None
        if transitions:
            try:
                self._before()
                pglib.transitions_enable(self.L, h)
                self._after()
                self.transitions = TransitionTensors(self)
            except Exception:
                self.close()
                raise

    # -- life cycle ------------------------------------------------------------------------------
    def reset(self, mask=None, seeds=None):
        """cenv_reset on every env (or those with mask != 0); seeds (int32[N]) reseed the streams."""
        m = None
        s = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        if seeds is not None:
            s = torch.as_tensor(seeds, device=self.device).to(torch.int32).contiguous()
        self._before()
        pglib.check(self.L, self.L.pgv_reset(self._h, c_void_p(m.data_ptr()) if m is not None else None,
                                             c_void_p(s.data_ptr()) if s is not None else None), "pgv_reset")
        self._after()
        self._keep = (m, s)
        return self.obs

    def step(self, actions):
        """actions: int32[N] tensor on this device (or anything torch.as_tensor accepts).
        Returns (obs u8[N,64,64,3], reward f32[N], done u8[N]) — views of the engine's buffers, valid
        until the next step; work is enqueued on torch's current stream."""
        a = torch.as_tensor(actions, device=self.device).to(torch.int32).contiguous()
        if a.numel() != self.num_envs:
            raise ValueError("expected %d actions, got %d" % (self.num_envs, a.numel()))
        self._before()
        pglib.check(self.L, self.L.pgv_step(self._h, c_void_p(a.data_ptr())), "pgv_step")
        self._after()
        self._keep = (a,)
        return self.obs, self.reward, self.done

    def step_synthetic(self, run_seed=0, ordered=True):
        """One step with device-generated actions.  ordered=False skips the stream hand-shake with the caller's current
        stream (several envs stepping side by side on their own streams; call sync() before reading the outputs)."""
        if ordered:
            self._before()
        pglib.check(self.L, self.L.pgv_step_synthetic(self._h, run_seed), "pgv_step_synthetic")
        if ordered:
            self._after()
        return self.obs, self.reward, self.done

    def _needs_episodes(self):
        if self.episode is None:
            raise pglib.EngineError("step_episodes needs an env made with autoreset_mode='next_step' or 'same_step'")

    def step_episodes(self, actions):
        """step() with the episode bookkeeping of the mode this env was made with (pgv_step_episodes): one engine call, no
        host synchronisation.  Returns (obs, episode): in same_step mode the obs rows of the envs that ended already show
        their next episode's first frame; `episode` (also self.episode) holds this step's reward / terminated / truncated /
        ended, the list of ended envs with their returns, lengths and levels, and the ring of terminal frames — views of
        the engine's buffers, reused by the next step_episodes."""
        self._needs_episodes()
        a = torch.as_tensor(actions, device=self.device).to(torch.int32).contiguous()
        if a.numel() != self.num_envs:
            raise ValueError("expected %d actions, got %d" % (self.num_envs, a.numel()))
        self._before()
        pglib.check(self.L, self.L.pgv_step_episodes(self._h, c_void_p(a.data_ptr())), "pgv_step_episodes")
        self._after()
        self._keep = (a,)
        return self.obs, self.episode

    def step_episodes_synthetic(self, run_seed=0, ordered=True):
        """step_synthetic() with the episode bookkeeping (pgv_step_episodes_synthetic); ordered as there."""
        self._needs_episodes()
        if ordered:
            self._before()
        pglib.check(self.L, self.L.pgv_step_episodes_synthetic(self._h, run_seed), "pgv_step_episodes_synthetic")
        if ordered:
            self._after()
        return self.obs, self.episode

    def step_episodes_times(self, steps, run_seed=0):
        """`steps` step_episodes_synthetic calls timed by HIP events on the engine's stream (pgv_step_episodes_times):
        (step_ms[steps], episode_ms[steps]) — the whole call, and the two episode launches behind the step alone."""
        import numpy as np
        self._needs_episodes()
        step_ms, episode_ms = np.zeros(steps, np.float32), np.zeros(steps, np.float32)
        pglib.check(self.L, self.L.pgv_step_episodes_times(self._h, steps, run_seed, c_void_p(step_ms.ctypes.data),
                                                           c_void_p(episode_ms.ctypes.data)), "pgv_step_episodes_times")
        return step_ms, episode_ms

    # -- steps without frames (include/procgen2_vec.h pgv_step_sequence) ---------------------------
    def step_sequence(self, actions=None, steps=None, *, frames="last", run_seed=0, rewards=True, dones=True, summary=True,
                      out=None):
        """T sub-steps in one engine call, of which only the last is drawn (frames="last") or none (frames="none").
        actions: int32 [T, N] — sub-step t plays row t — or int32 [N] with steps=T, the same row every sub-step (action
        repeat), or None with steps=T for device-generated actions (run_seed; the hash and step counter of step_synthetic).
        The engine is left as T step() calls would leave it; an env that reports done inside the sequence serves its reset
        in the next sub-step and plays on.

        Returns a SequenceResult: obs (the engine's obs view; None with frames="none" — render_obs() draws it when wanted),
        rewards f32 [T, N] and dones u8 [T, N] (what reward / done held after each sub-step), seq_length i32 [N] (sub-steps
        up to and including the env's first done, T without one), seq_done u8 [N] (whether there was one) and seq_return
        f32 [N] (the float32 sum of the env's rewards over those sub-steps, in order).  rewards / dones / summary = False
        leave the respective parts out (None).  The tensors live on this env's device, are allocated once per T and written
        again by the next call with the same T; the sets of the four most recently used T are kept (5·T·N + 9·N bytes each),
        an older one is dropped and allocated afresh when its T comes again.  A caller whose T varies widely passes out = a
        SequenceResult of caller-owned contiguous tensors of those shapes to write instead.  Same stream hand-shake as step(), no host synchronisation."""
        if frames not in pglib.FRAMES:
            raise ValueError("frames must be 'last' or 'none'")
        n, a, stride = self.num_envs, None, 0
        if actions is not None:
            a = torch.as_tensor(actions, device=self.device).to(torch.int32).contiguous()
            if a.dim() == 2 and a.shape[1] == n and steps in (None, a.shape[0]):
                steps, stride = a.shape[0], n
            elif not (a.dim() == 1 and a.numel() == n and steps is not None):
                raise ValueError("step_sequence: actions must be [T, %d], or [%d] with steps=T" % (n, n))
        elif steps is None:
            raise ValueError("step_sequence: steps is needed without [T, N] actions")
        T = int(steps)
        if T < 0:
            raise ValueError("step_sequence: steps must be >= 0")
        want = SequenceResult.layout(T, n)
        if out is None:
            out = self._sequences.pop(T, None)
            if out is None:
                out = SequenceResult(**{k: torch.zeros(shape, dtype=dtype, device=self.device) for k, (shape, dtype) in want.items()})
            self._sequences[T] = out  # (most recent last)
            while len(self._sequences) > _SEQUENCES_KEPT:
                del self._sequences[next(iter(self._sequences))]
        else:
            for k, (shape, dtype) in want.items():
                t = getattr(out, k)
                if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous()):
                    raise ValueError("out.%s: expected a contiguous %s tensor of shape %s on %s" % (k, dtype, shape, self.device))
        given = {"rewards": rewards, "dones": dones, "seq_return": summary, "seq_length": summary, "seq_done": summary}
        res = SequenceResult(**{k: getattr(out, k) if given[k] else None for k in want})
        ptr = {k: c_void_p(getattr(res, k).data_ptr()) if getattr(res, k) is not None and T else None for k in want}
        seq = pglib.sequence(T, c_void_p(a.data_ptr()) if a is not None else None, stride, run_seed, frames, **ptr)
        self._before()
        pglib.check(self.L, self.L.pgv_step_sequence(self._h, ctypes.byref(seq)), "pgv_step_sequence")
        self._after()
        self._keep = (a, res)
        res.obs = self.obs if frames == "last" else None
        return res

    def render_obs(self, mask=None):
        """Draw the observations of the state as it stands (pgv_render_obs) — after step_sequence(frames="none"), or at any
        time between steps: no state changes.  mask (uint8 [N], non-zero = draw): the other rows keep their bytes.  Returns
        the obs view."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            if m.numel() != self.num_envs:
                raise ValueError("expected a mask of %d envs, got %d" % (self.num_envs, m.numel()))
        self._before()
        pglib.check(self.L, self.L.pgv_render_obs(self._h, c_void_p(m.data_ptr()) if m is not None else None), "pgv_render_obs")
        self._after()
        self._keep = (m,)
        return self.obs

    def push_policy_obs(self, mask=None):
        """Push the obs slab as it stands into the policy tensor by hand (pgv_policy_obs_push) — after
        step_sequence(frames="none") and render_obs(), say; step(), reset() and the drawn sequences push on their own.
        mask (uint8 [N], non-zero = push): the other envs keep their stacks and their restart flags.  Returns policy_obs."""
        if self.policy_obs is None:
            raise pglib.EngineError("push_policy_obs needs an env made with policy_obs=dict(...)")
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
            if m.numel() != self.num_envs:
                raise ValueError("expected a mask of %d envs, got %d" % (self.num_envs, m.numel()))
        self._before()
        pglib.check(self.L, self.L.pgv_policy_obs_push(self._h, c_void_p(m.data_ptr()) if m is not None else None), "pgv_policy_obs_push")
        self._after()
        self._keep = (m,)
        return self.policy_obs

    def _needs_history(self, who):
        if self.history is None:
            raise pglib.EngineError(who + " needs an env made with history=dict(capacity=T, ...)")

    def history_push(self):
        """Push the obs slab as it stands into a new slot of the frame history by hand (pgv_history_push), all envs — after
        step_sequence(frames="none") and render_obs(), say; step(), step_episodes() and the drawn sequences push on their
        own.  Returns the push number of the slot it wrote."""
        self._needs_history("history_push")
        self._before()
        pglib.check(self.L, self.L.pgv_history_push(self._h), "pgv_history_push")
        self._after()
        return self.history.head - 1

    def history_gather(self, pushes, envs, stack=4, dtype="float16", out=None, augment=None, return_params=False):
        """Rows [B, K*C, 64, 64] of `dtype` ("uint8", "float16", "bfloat16", "float32") for the B pairs (pushes[b], envs[b])
        — int64 and int32 device tensors, or anything torch.as_tensor takes: row slot K-1 is the frame of that push, the
        slots in front of it the env's frames before it, never across the start of an episode nor past the oldest push held
        (pgv_history_gather).  A pair whose push is not held (head - T <= p < head) or whose env is outside the batch gives a
        row of zeros.  out: a caller-owned contiguous tensor of that shape and dtype to write into (and return).  Same stream
        hand-shake as step(), no host synchronisation.

        augment = None | dict(size=int | (H, W), pad=0, edge="replicate" | "zero", cutout=None | (lo, hi),
        cutout_color="black" | "random", seed=int): the rows through a random window and a cutout, drawn per row from `seed`
        and the row's position, on the stored bytes (pgv_history_gather_aug): [B, K*C, H', W'].  size: H' in 1 .. 64, W' in
        8 .. 64 and a multiple of 8; pad 0 .. 16: how far a window may hang over the frame, where `edge` fills in; cutout:
        the range of the rectangle's sides, 1 <= lo <= hi <= 64.  seed is required: the same seed gives the same rows.
        return_params=True: (rows, params int32 [B, 8]) — oy, ox, cy, cx, ch, cw, colour, 0 of every row."""
        aug = None if augment is None else _augment_config(augment)
        if return_params and aug is None:
            raise ValueError("history_gather: return_params needs augment=dict(...)")
        self._needs_history("history_gather")
        if dtype not in pglib.POLICY_DTYPES:
            raise ValueError("history_gather: dtype must be one of %s" % ", ".join(pglib.POLICY_DTYPES))
        if isinstance(stack, bool) or not isinstance(stack, int) or not 1 <= stack <= 8:
            raise ValueError("history_gather: stack must be an integer in 1 .. 8")
        p = torch.as_tensor(pushes, device=self.device).to(torch.int64).reshape(-1).contiguous()
        i = torch.as_tensor(envs, device=self.device).to(torch.int32).reshape(-1).contiguous()
        if p.numel() != i.numel():
            raise ValueError("history_gather: %d pushes but %d envs" % (p.numel(), i.numel()))
        shape = (p.numel(), stack * self.history.frames.shape[2]) + ((64, 64) if aug is None else (aug.out_height, aug.out_width))
        tdtype = getattr(torch, dtype)
        if out is None:
            out = torch.empty(shape, dtype=tdtype, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != tdtype or out.device != self.device or not out.is_contiguous():
            raise ValueError("out: expected a contiguous %s tensor of shape %s on %s" % (tdtype, shape, self.device))
        params = torch.empty((p.numel(), 8), dtype=torch.int32, device=self.device) if return_params else None
        if p.numel():
            self._before()
            if aug is None:
                pglib.check(self.L, self.L.pgv_history_gather(self._h, c_void_p(p.data_ptr()), c_void_p(i.data_ptr()), p.numel(), stack,
                                                              pglib.POLICY_DTYPES[dtype][0], c_void_p(out.data_ptr())), "pgv_history_gather")
            else:
                aug.params = params.data_ptr() if return_params else None
                pglib.check(self.L, self.L.pgv_history_gather_aug(self._h, c_void_p(p.data_ptr()), c_void_p(i.data_ptr()), p.numel(), stack,
                                                                  pglib.POLICY_DTYPES[dtype][0], ctypes.byref(aug), c_void_p(out.data_ptr())),
                            "pgv_history_gather_aug")
            self._after()
            self._keep_gather = (p, i, out, params)
        return (out, params) if return_params else out

    def _needs_transitions(self, who):
        if self.transitions is None:
            raise pglib.EngineError(who + " needs an env made with history=dict(capacity=T, ...), transitions=True")

    def transition_gather(self, pushes, envs, n=3, gamma=0.99, stack=4, dtype="float16", frames=True):
        """The n-step transitions of the B pairs (pushes[b], envs[b]) in one launch (pgv_transitions_gather): a Transition of
        obs and next_obs [B, K*C, 64, 64] of `dtype` — history_gather's rows for push p and for push p + steps —, action int32
        [B], nstep_return and discount float32 [B] (discount 0 behind a terminal step, else gamma ** steps, rounded per step),
        steps int32 [B] (the rows actually folded: fewer than n at an episode's end or the ring's), status u8 [B] (bit 0 valid,
        pglib.TR_TERMINATED / TR_TRUNCATED / TR_CUT of the last row folded).  A pair whose row is not held with its
        successor, not recorded or a reset's own step, or whose env is outside the batch, gives zeros.  frames=False: the
        scalars alone (obs and next_obs None).  Same stream hand-shake as step(), no host synchronisation."""
        self._needs_transitions("transition_gather")
        if dtype not in pglib.POLICY_DTYPES:
            raise ValueError("transition_gather: dtype must be one of %s" % ", ".join(pglib.POLICY_DTYPES))
        if isinstance(stack, bool) or not isinstance(stack, int) or not 1 <= stack <= 8:
            raise ValueError("transition_gather: stack must be an integer in 1 .. 8")
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 64:
            raise ValueError("transition_gather: n must be an integer in 1 .. 64")
        p = torch.as_tensor(pushes, device=self.device).to(torch.int64).reshape(-1).contiguous()
        i = torch.as_tensor(envs, device=self.device).to(torch.int32).reshape(-1).contiguous()
        if p.numel() != i.numel():
            raise ValueError("transition_gather: %d pushes but %d envs" % (p.numel(), i.numel()))
        B = p.numel()
        shape = (B, stack * self.history.frames.shape[2], 64, 64)
        obs = torch.empty(shape, dtype=getattr(torch, dtype), device=self.device) if frames else None
        next_obs = torch.empty(shape, dtype=getattr(torch, dtype), device=self.device) if frames else None
        action = torch.empty(B, dtype=torch.int32, device=self.device)
        ret = torch.empty(B, dtype=torch.float32, device=self.device)
        discount = torch.empty(B, dtype=torch.float32, device=self.device)
        steps = torch.empty(B, dtype=torch.int32, device=self.device)
        status = torch.empty(B, dtype=torch.uint8, device=self.device)
        if B:
            q = pglib.transition_query(n, gamma, stack, dtype, obs.data_ptr() if frames else None, next_obs.data_ptr() if frames else None,
                                       action.data_ptr(), ret.data_ptr(), discount.data_ptr(), steps.data_ptr(), status.data_ptr())
            self._before()
            pglib.check(self.L, self.L.pgv_transitions_gather(self._h, c_void_p(p.data_ptr()), c_void_p(i.data_ptr()), B, ctypes.byref(q)),
                        "pgv_transitions_gather")
            self._after()
            self._keep_transitions = (p, i, obs, next_obs, action, ret, discount, steps, status)
        return Transition(obs, next_obs, action, ret, discount, steps, status)

    def transition_gae(self, first, steps, values, gamma=0.999, lam=0.95, trunc_values=None):
        """(advantages, returns), float32 [steps, N], of the GAE recurrence over rows first .. first + steps - 1 of the record
        ring in one launch (pgv_transitions_gae): values float32 [steps + 1, N] (the last row bootstraps), trunc_values
        float32 [steps, N] or None: the value of the state a truncated step ended in (None: 0).  Every row must be held with
        its successor: head - T <= q and q + 1 < head.  Terminal, truncated and cut rows end the recurrence; rows that are
        not recorded, and a reset's own step, give advantage 0 and return V."""
        self._needs_transitions("transition_gae")
        steps = int(steps)
        n = self.num_envs

        def rows(x, count, name):
            x = torch.as_tensor(x, device=self.device).to(torch.float32).contiguous()
            if tuple(x.shape) != (count, n):
                raise ValueError("transition_gae: %s must have shape (%d, %d)" % (name, count, n))
            return x
        if steps < 1:
            raise ValueError("transition_gae: steps must be >= 1")
        v = rows(values, steps + 1, "values")
        tv = None if trunc_values is None else rows(trunc_values, steps, "trunc_values")
        adv = torch.empty((steps, n), dtype=torch.float32, device=self.device)
        ret = torch.empty((steps, n), dtype=torch.float32, device=self.device)
        g = pglib.gae(gamma, lam, v.data_ptr(), adv.data_ptr(), None if tv is None else tv.data_ptr(), ret.data_ptr())
        self._before()
        pglib.check(self.L, self.L.pgv_transitions_gae(self._h, int(first), steps, ctypes.byref(g)), "pgv_transitions_gae")
        self._after()
        self._keep_gae = (v, tv, adv, ret)
        return adv, ret

    def _before(self):
        self._stream.wait_stream(torch.cuda.current_stream(self.device))

    def _after(self):
        torch.cuda.current_stream(self.device).wait_stream(self._stream)

    def timed_steps(self, steps, run_seed=0, render_events=True):
        """(total_ms, render_kernel_ms_sum) from HIP events on the engine's stream.  render_events=False: the region holds
        the steps and nothing else (no event pair per render launch); the second value is then None."""
        total, render = ctypes.c_double(), ctypes.c_double()
        pglib.check(self.L, self.L.pgv_timed_steps(self._h, steps, run_seed, ctypes.byref(total),
                                                   ctypes.byref(render) if render_events else None), "pgv_timed_steps")
        return total.value, (render.value if render_events else None)

    def step_times(self, steps, run_seed=0):
        """Per-step detail of `steps` synthetic steps (HIP events on the engine's stream): (step_ms[steps],
        render_ms[steps]) as numpy float32 arrays — for latency percentiles and the roofline window."""
        import numpy as np
        step_ms, render_ms = np.zeros(steps, np.float32), np.zeros(steps, np.float32)
        pglib.check(self.L, self.L.pgv_step_times(self._h, steps, run_seed, c_void_p(step_ms.ctypes.data),
                                                  c_void_p(render_ms.ctypes.data)), "pgv_step_times")
        return step_ms, render_ms

    def step_phases(self, steps, run_seed=0):
        """`steps` synthetic steps cut into their phases by HIP events on the engine's stream (include/procgen2_vec.h
        pgv_step_phases): a dict of numpy float32 arrays step / logic / prepass / render / late, milliseconds per step;
        logic + prepass + render + late = step."""
        import numpy as np
        names = ("step", "logic", "prepass", "render", "late")
        out = {k: np.zeros(steps, np.float32) for k in names}
        pglib.check(self.L, self.L.pgv_step_phases(self._h, steps, run_seed, *(c_void_p(out[k].ctypes.data) for k in names)),
                    "pgv_step_phases")
        return out

    def render_frame(self, index=0, width=512, height=512):
        """The human-size frame of env `index` (cenv_render, render_game(false)): uint8 [height, width, 3] on the host."""
        import numpy as np
        out = np.zeros((height, width, 3), np.uint8)
        pglib.check(self.L, self.L.pgv_render_frame(self._h, index, width, height, c_void_p(out.ctypes.data)),
                    "pgv_render_frame")
        return out

    def render_frames(self, indices=None, width=512, height=512, out=None):
        """The human-size frames of the envs `indices` (None: all of them, in order; otherwise anything torch.as_tensor
        takes — an env may appear more than once, an index outside the batch gives a frame of zeros): uint8
        [K, height, width, 3] on this env's device, rendered there in one batched call (pgv_render_frames) with the same
        stream hand-shake as step() and no host synchronisation.  out: a caller-owned contiguous tensor of that shape to
        write into (and return)."""
        width, height = int(width), int(height)
        idx = None
        count = self.num_envs
        if indices is not None:
            idx = torch.as_tensor(indices, device=self.device).to(torch.int32).reshape(-1).contiguous()
            count = idx.numel()
        shape = (count, height, width, 3)
        if out is None:
            if not (1 <= width <= 4096 and 1 <= height <= 4096):
                raise ValueError("render_frames: width and height must be in 1..4096")
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous():
            raise ValueError("out: expected a contiguous %s tensor of shape %s on %s" % (torch.uint8, shape, self.device))
        if count:
            self._before()
            pglib.check(self.L, self.L.pgv_render_frames(self._h, c_void_p(idx.data_ptr()) if idx is not None else None,
                                                         count, width, height, c_void_p(out.data_ptr())), "pgv_render_frames")
            self._after()
            self._keep_frames = (idx, out)
        return out

    # -- symbolic observations (include/procgen2_vec.h pgv_state_rows / pgv_tile_rows) ------------
    def _obs_out(self, out, shape, dtype, name):
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if (tuple(out.shape) != shape or out.dtype != dtype or out.device != self.device or not out.is_contiguous()
                or out.data_ptr() % 16):
            raise ValueError("%s: expected a contiguous, 16-byte aligned %s tensor of shape %s on %s" % (name, dtype, shape, self.device))
        return out

    def state_obs(self, envs=None, out=None, lengths_out=None):
        """What the game knows about the envs `envs` (None: all of them, in order; otherwise anything torch.as_tensor takes —
        an env may appear more than once, an index outside the batch gives a row of zeros and length 0), as it stands now:
        (rows float32 [B, state_layout.width], lengths int32 [B]) on this env's device.  Row k is the env's state dump —
        state_layout.fixed_names, then lengths[k] - fixed floats of records of state_layout.record_names — and +0.0 behind
        it.  Written on the device with the same stream hand-shake as step() and no host synchronisation; reads only.
        out / lengths_out: caller-owned contiguous tensors of those shapes to write into (and return)."""
        idx, count = self._indices(envs)
        out = self._obs_out(out, (count, self.state_layout.width), torch.float32, "out")
        lengths_out = self._obs_out(lengths_out, (count,), torch.int32, "lengths_out")
        if count:
            self._before()
            pglib.check(self.L, self.L.pgv_state_rows(self._h, c_void_p(idx.data_ptr()) if idx is not None else None, count,
                                                      c_void_p(out.data_ptr()), c_void_p(lengths_out.data_ptr())), "pgv_state_rows")
            self._after()
            self._keep_state_obs = (idx, out, lengths_out)
        return out, lengths_out

    def tile_obs(self, envs=None, out=None):
        """The tile maps of the envs `envs` (as state_obs takes them): uint8 [B, state_layout.cells] on this env's device,
        cell (x, y) at column y + x * state_layout.tile_h — [B, 0] for a game without a tile map (bossfight).  An index
        outside the batch gives a row of zeros.  out: a caller-owned contiguous tensor of that shape to write into."""
        idx, count = self._indices(envs)
        out = self._obs_out(out, (count, self.state_layout.cells), torch.uint8, "out")
        if count and self.state_layout.cells:
            self._before()
            pglib.check(self.L, self.L.pgv_tile_rows(self._h, c_void_p(idx.data_ptr()) if idx is not None else None, count,
                                                     c_void_p(out.data_ptr())), "pgv_tile_rows")
            self._after()
            self._keep_tile_obs = (idx, out)
        return out

    # -- path distances (include/procgen2_vec.h pgv_tile_paths_rows) -----------------------------
    def tile_paths(self, source="goal", probe="agent", passable=(0,), envs=None, source_cells=None, probe_cells=None, dist=True,
                   out=None):
        """Breadth-first path distances over the tile maps of the envs `envs` (as state_obs takes them), as they stand now.
        The field is a geometric distance over cells (the platformers' physics are not in it).

        source: "agent", "goal" or "cells"; probe: "none", "agent", "goal" or "cells".  The agent's cell is the cell of the
        centre of its body box, (agent_x, agent_y + path_layout.agent_dy); the goal's that of goal_x, goal_y (maze,
        jumper) or of entity 0 (caveflyer) — "goal" is refused for the other games.  "cells" takes source_cells /
        probe_cells: int32 [B], cell (x, y) = y + x * tile_h as in tile_obs, a value outside 0 .. cells-1 meaning no cell.
        passable: the tile ids (as tile_obs gives them, below 32) that may be entered, as an iterable or a 32-bit mask.
        The source cell has distance 0 whatever its tile; a cell has distance d + 1 when it is passable, not yet reached and
        has a 4-neighbour at distance d; no wrap at any edge; every other cell is -1.

        Returns a TilePaths on this env's device: dist int16 [B, cells] (None with dist=False), probe_dist int32 [B] (-1:
        not reached, or no probe cell), probe_step uint8 [B] (0 where probe_dist <= 0, else the first of x-1 (1), x+1 (2),
        y-1 (3), y+1 (4) whose distance is one less) and cells int32 [B, 2] (source cell, probe cell; -1 for none).  A row
        without a source, or of an env outside the batch, is -1 everywhere with step 0.  out: a caller-owned contiguous,
        16-byte aligned int16 [B, cells] tensor for dist.  Same stream hand-shake as tile_obs(), no host synchronisation;
        reads only.  In maze, torch.tensor(procgen2_amd.MAZE_STEP_ACTIONS)[paths.probe_step.long()] with the defaults is
        the optimal policy."""
        for name, value, kinds in (("source", source, ("agent", "goal", "cells")), ("probe", probe, ("none", "agent", "goal", "cells"))):
            if value not in kinds:
                raise ValueError("%s must be one of %s, not %r" % (name, ", ".join(kinds), value))
        idx, count = self._indices(envs)
        cells = self.path_layout.cells
        given = []
        for name, kind, value in (("source_cells", source, source_cells), ("probe_cells", probe, probe_cells)):
            if kind != "cells":
                given.append(None)
                continue
            if value is None:
                raise ValueError("%s is needed with %s='cells'" % (name, name[:-6]))
            value = torch.as_tensor(value, device=self.device).to(torch.int32).reshape(-1).contiguous()
            if value.numel() != count:
                raise ValueError("%s: expected %d cells, got %d" % (name, count, value.numel()))
            given.append(value)
        if out is not None and not dist:
            raise ValueError("out is given with dist=False")
        res = TilePaths(dist=self._obs_out(out, (count, cells), torch.int16, "out") if dist else None,
                        probe_dist=torch.empty((count,), dtype=torch.int32, device=self.device),
                        probe_step=torch.empty((count,), dtype=torch.uint8, device=self.device),
                        cells=torch.empty((count, 2), dtype=torch.int32, device=self.device))
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        q = pglib.TilePathsStruct(ctypes.sizeof(pglib.TilePathsStruct), pglib.passable_mask(passable), pglib.PATH_POINTS[source],
                                  ptr(given[0]), pglib.PATH_POINTS[probe], ptr(given[1]), ptr(res.dist), ptr(res.probe_dist),
                                  ptr(res.probe_step), ptr(res.cells))
        self._before()
        pglib.check(self.L, self.L.pgv_tile_paths_rows(self._h, c_void_p(idx.data_ptr()) if idx is not None and count else None, count,
                                                       ctypes.byref(q)), "pgv_tile_paths_rows")
        self._after()
        self._keep_tile_paths = (idx, given, res)
        return res

    # -- caller-made levels (include/procgen2_vec.h pgv_get_levels / pgv_set_levels) -----------------
    def _needs_levels(self, who):
        if not self.level_layout.supported:
            raise pglib.EngineError("%s: no caller-made levels for this game (%s)" % (who, self.game))

    def get_levels(self, envs=None, host=False):
        """The levels of the envs `envs` (as state_obs takes them) as they stand now, the agent's current cell included: a
        Levels of tiles uint8 [B, level_layout.cells] (0 open, 1 wall; cell (x, y) at column y + x * tile_h, as tile_obs),
        agent_cell and goal_cell int32 [B], background int32 [B] (the floor picture, 0 .. level_layout.backgrounds - 1) and
        background_shift float32 [B].  An index outside the batch gives a zero tile row and cells of -1.  Device tensors,
        written there with the same stream hand-shake as step() and no host synchronisation; reads only.  host=True: numpy
        arrays through the synchronous host form (envs then anything numpy takes).  maze only (level_layout.supported)."""
        self._needs_levels("get_levels")
        cells = self.level_layout.cells
        if host:
            import numpy as np
            idx = None if envs is None else np.ascontiguousarray(np.asarray(envs).reshape(-1), np.int32)
            count = self.num_envs if idx is None else idx.size
            res = Levels(np.zeros((count, cells), np.uint8), np.zeros(count, np.int32), np.zeros(count, np.int32),
                         np.zeros(count, np.int32), np.zeros(count, np.float32))
            rows = pglib.level_rows(*(x.ctypes.data if count else None for x in res))
            pglib.check(self.L, self.L.pgv_get_levels_host(self._h, c_void_p(idx.ctypes.data) if idx is not None and count else None,
                                                           count, ctypes.byref(rows)), "pgv_get_levels_host")
            return res
        idx, count = self._indices(envs)
        res = Levels(torch.empty((count, cells), dtype=torch.uint8, device=self.device),
                     torch.empty((count,), dtype=torch.int32, device=self.device), torch.empty((count,), dtype=torch.int32, device=self.device),
                     torch.empty((count,), dtype=torch.int32, device=self.device), torch.empty((count,), dtype=torch.float32, device=self.device))
        if count:
            rows = pglib.level_rows(*(x.data_ptr() for x in res))
            self._before()
            pglib.check(self.L, self.L.pgv_get_levels(self._h, c_void_p(idx.data_ptr()) if idx is not None else None, count,
                                                      ctypes.byref(rows)), "pgv_get_levels")
            self._after()
            self._keep_get_levels = (idx, res)
        return res

    def set_levels(self, levels=None, *, tiles=None, agent_cell=None, goal_cell=None, background=None, background_shift=None,
                   ids=None, indices=None):
        """Install caller-made levels as the start of a new episode of the envs `indices` (None: row k into env k; otherwise
        distinct indices, one outside the batch gives status 1).  levels: a Levels (what get_levels returns, edited in torch),
        or the fields by keyword — tiles uint8 [B, cells] of 0 (open) and 1 (wall), agent_cell and goal_cell int32 [B]; with
        background / background_shift None every env keeps the floor it has; ids uint32 labels [B] that level_numbers shows
        (level_known is 2 for a caller-made level), 0 without.  A keyword overrides the field of `levels`.

        Returns status int32 [B]: 0 installed, 1 no such env, 2 a tile byte that is neither 0 nor 1, 3 / 4 the agent's / the
        goal's cell outside the map, on a wall (or the goal on the agent), 5 a background outside 0 .. backgrounds - 1 or a
        shift outside [0, 1).  A refused row leaves its env untouched.  An installed env is as after reset(): obs shows the
        level's first frame, reward and done are 0, stacks, history and running episode values restart; its random stream,
        its prefetched next level and a pending assignment stay, so the level after the custom one is the one it would have
        built anyway.  Device tensors stay on the device: same stream hand-shake as step(), no host synchronisation.  When
        `tiles` is a numpy array the synchronous host form is used and status is a numpy array.  maze only."""
        self._needs_levels("set_levels")
        if levels is not None:
            tiles = levels.tiles if tiles is None else tiles
            agent_cell = levels.agent_cell if agent_cell is None else agent_cell
            goal_cell = levels.goal_cell if goal_cell is None else goal_cell
            background = levels.background if background is None else background
            background_shift = levels.background_shift if background_shift is None else background_shift
        if tiles is None or agent_cell is None or goal_cell is None:
            raise ValueError("set_levels: tiles, agent_cell and goal_cell are needed")
        cells = self.level_layout.cells
        host = not torch.is_tensor(tiles)
        if host:
            import numpy as np
            as_rows = lambda x, dtype: None if x is None else np.ascontiguousarray(np.asarray(x).reshape(-1), dtype)
            t = np.ascontiguousarray(tiles, np.uint8).reshape(-1, cells)
        else:
            as_rows = lambda x, dtype: None if x is None else torch.as_tensor(x, device=self.device).to(getattr(torch, dtype)).reshape(-1).contiguous()
            t = tiles.to(device=self.device, dtype=torch.uint8).reshape(-1, cells).contiguous()
        count = t.shape[0]
        label = ids
        if label is not None and not host:  # (the 32-bit pattern: torch lacks most uint32 ops)
            label = torch.as_tensor(label, device=self.device)
            if label.dtype == torch.uint32:
                label = label.view(torch.int32)
            elif label.dtype != torch.int32:
                label = label.to(torch.int64) & 0xFFFFFFFF
                label = torch.where(label >= 1 << 31, label - (1 << 32), label).to(torch.int32)
        given = {"agent_cell": as_rows(agent_cell, "int32"), "goal_cell": as_rows(goal_cell, "int32"),
                 "background": as_rows(background, "int32"), "background_shift": as_rows(background_shift, "float32"),
                 "ids": as_rows(label, "uint32" if host else "int32"), "indices": as_rows(indices, "int32")}
        for name, x in given.items():
            if x is not None and (x.size if host else x.numel()) != count:
                raise ValueError("set_levels: %s has %d entries for %d tile rows" % (name, x.size if host else x.numel(), count))
        if indices is None and count != self.num_envs:
            raise ValueError("set_levels: expected %d levels, got %d (or give indices)" % (self.num_envs, count))
        if host:
            status = np.zeros(count, np.int32)
            ptr = lambda x: x.ctypes.data if x is not None and count else None
        else:
            status = torch.zeros((count,), dtype=torch.int32, device=self.device)
            ptr = lambda x: x.data_ptr() if x is not None and count else None
        rows = pglib.level_rows(ptr(t), ptr(given["agent_cell"]), ptr(given["goal_cell"]), ptr(given["background"]),
                                ptr(given["background_shift"]), ptr(given["ids"]), ptr(status))
        call, name = (self.L.pgv_set_levels_host, "pgv_set_levels_host") if host else (self.L.pgv_set_levels, "pgv_set_levels")
        self._before()
        pglib.check(self.L, call(self._h, c_void_p(ptr(given["indices"])), count, ctypes.byref(rows)), name)
        self._after()
        self._keep_set_levels = (t, given, status)
        return status

    def save_state(self):
        """Snapshot of the whole batch (state, RNG streams, prefetched levels, outputs) as a numpy byte array."""
        import numpy as np
        n = self.L.pgv_snapshot_bytes(self._h)
        buf = np.empty(n, np.uint8)
        pglib.check(self.L, self.L.pgv_save_state(self._h, c_void_p(buf.ctypes.data), n), "pgv_save_state")
        return buf

    def load_state(self, buf):
        import numpy as np
        buf = np.ascontiguousarray(buf, np.uint8)
        pglib.check(self.L, self.L.pgv_load_state(self._h, c_void_p(buf.ctypes.data), buf.size), "pgv_load_state")
        if self.policy_obs is not None or self.history is not None:  # (the flags the load sets on the engine's stream, ordered for the caller)
            self._after()

    # -- per-env records (include/procgen2_vec.h pgv_save_envs / pgv_load_envs) -------------------
    @property
    def env_record_bytes(self):
        return int(self.L.pgv_env_record_bytes(self._h))

    @property
    def env_record_tag(self):
        return int(self.L.pgv_env_record_tag(self._h))

    def _indices(self, indices):
        if indices is None:
            return None, self.num_envs
        idx = torch.as_tensor(indices, device=self.device).to(torch.int32).reshape(-1).contiguous()
        return idx, idx.numel()

    def save_envs(self, indices=None, out=None):
        """The state records of the envs `indices` (None: all of them, in order; otherwise anything torch.as_tensor takes —
        an env may appear more than once, an index outside the batch gives an empty record) as an EnvRecords: uint8
        [K, env_record_bytes] on this env's device plus the configuration's tag.  Gathered on the device with the same
        stream hand-shake as step() and no host synchronisation.  out: a caller-owned contiguous uint8 tensor of that
        shape to write into (it becomes the result's `data`)."""
        idx, count = self._indices(indices)
        shape = (count, self.env_record_bytes)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif (tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous()
              or out.data_ptr() % 16):
            raise ValueError("out: expected a contiguous, 16-byte aligned %s tensor of shape %s on %s" % (torch.uint8, shape, self.device))
        if count:
            self._before()
            pglib.check(self.L, self.L.pgv_save_envs(self._h, c_void_p(idx.data_ptr()) if idx is not None else None, count,
                                                     c_void_p(out.data_ptr())), "pgv_save_envs")
            self._after()
            self._keep_records = (idx, out)
        return EnvRecords(out, self.env_record_tag)

    def load_envs(self, records, indices=None):
        """Put `records` (an EnvRecords of an env of the same configuration on this device) into the slots `indices`
        (None: record k into slot k; the indices must be distinct, one outside the batch is skipped, and so is an empty
        record).  From here on each slot goes on as the env it was saved from; obs / reward / done show its rows at the
        save.  Records of another configuration raise EngineError and change nothing."""
        data = records.data
        if data.dtype != torch.uint8 or data.dim() != 2 or data.device != self.device:
            raise ValueError("load_envs: records.data must be a uint8 [K, record_bytes] tensor on %s" % self.device)
        if data.shape[1] != self.env_record_bytes and records.tag == self.env_record_tag:
            raise ValueError("load_envs: records of %d bytes, this env's are %d" % (data.shape[1], self.env_record_bytes))
        if not data.is_contiguous() or data.data_ptr() % 16:
            data = data.clone(memory_format=torch.contiguous_format)
        idx, count = self._indices(indices)
        if indices is None:
            count = min(count, data.shape[0])
        elif count != data.shape[0]:
            raise ValueError("load_envs: %d indices for %d records" % (count, data.shape[0]))
        self._before()
        pglib.check(self.L, self.L.pgv_load_envs(self._h, c_void_p(idx.data_ptr()) if idx is not None else None, count,
                                                 c_void_p(data.data_ptr()), records.tag), "pgv_load_envs")
        self._after()
        self._keep_records = (idx, data)

    def fork(self, src, dst):
        """Copy env src[k] into slot dst[k] (save, then load): dst's slots go on as copies of the src envs.  An env may be
        a source many times; the destinations must be distinct.  Returns the records."""
        records = self.save_envs(src)
        self.load_envs(records, dst)
        return records

    # -- assigned levels (include/procgen2_vec.h pgv_assign_levels) --------------------------------
    def assign_levels(self, levels, indices=None):
        """Name the level each of the envs `indices` (None: env k gets levels[k]; otherwise distinct indices, one outside
        the batch is skipped) builds NEXT — at the auto-reset after its current episode, or at a reset() without seeds
        that names it.  Level number L is what level-seed mode means by it, whatever num_levels this env was made with: a
        fresh make(seed = L)'s first level.  levels / indices: anything torch.as_tensor takes (the low 32 bits of a level
        count); tensors on this device stay there.  Same stream hand-shake as step(), no host synchronisation.  A later
        assignment overwrites a pending one; reset(seeds=...) drops it.

        `level_numbers` (torch.uint32 [N]) and `level_known` (torch.uint8 [N]) are views of the engine's own buffers, as
        obs is: the number of the level each env is IN and whether it has one (level-seed mode or an assigned level; a
        free-mode level has known 0 and number 0).  They still name the finished level at the step that reports done and
        change with the new level's first frame.  uint32 because a level number is a 32-bit pattern; for the torch ops that
        lack uint32, `.view(torch.int32)` is the same bits and `.to(torch.int64)` the same values."""
        lv = torch.as_tensor(levels, device=self.device)
        if lv.dtype != torch.int32:  # (the 32-bit pattern, as the C ABI reads it: 2**32 - 1 and -1 name the same level)
            lv = lv.to(torch.int64) & 0xFFFFFFFF
            lv = torch.where(lv >= 1 << 31, lv - (1 << 32), lv).to(torch.int32)
        lv = lv.reshape(-1).contiguous()
        idx = None
        if indices is not None:
            idx = torch.as_tensor(indices, device=self.device).to(torch.int32).reshape(-1).contiguous()
            if idx.numel() != lv.numel():
                raise ValueError("assign_levels: %d indices for %d levels" % (idx.numel(), lv.numel()))
        elif lv.numel() != self.num_envs:
            raise ValueError("assign_levels: expected %d levels, got %d" % (self.num_envs, lv.numel()))
        if lv.numel():
            self._before()
            pglib.check(self.L, self.L.pgv_assign_levels(self._h, c_void_p(idx.data_ptr()) if idx is not None else None,
                                                         lv.numel(), c_void_p(lv.data_ptr())), "pgv_assign_levels")
            self._after()
            self._keep_levels = (idx, lv)

    def sync(self):
        pglib.check(self.L, self.L.pgv_sync(self._h), "pgv_sync")

    def publish(self):
        """Order torch's current stream behind the engine's stream (after step_synthetic(ordered=False)), without
        blocking the host: whatever is enqueued on the current stream next sees the step's outputs.  This covers
        read-after-write only: the NEXT unordered step would overwrite obs / reward / done while a reader enqueued here
        (a gather, a copy) is still at them — call consume() after enqueueing the readers."""
        self._after()

    def consume(self):
        """The counterpart of publish(): order the engine's stream behind torch's current stream, so the next
        step_synthetic(ordered=False) does not overwrite the outputs before what was enqueued on the current stream
        (and on streams it has been made to wait for, like a collective's) has read them."""
        self._before()

    def close(self):
        if self._h:
            self.L.pgv_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- multi-GPU -------------------------------------------------------------------------------
    def gather(self, dst=0, group=None):
        """Rooted gather of (obs, reward, done) to rank `dst` (a rank of `group`); other ranks get None.  Optional: the
        hot path itself never communicates.  The plan (per-rank env counts, the root's slabs) is made on the first call
        and reused: a call is then one batch of point-to-point transfers and no host synchronisation."""
        key = (dst, id(group))
        plan = self._gathers.get(key) if hasattr(self, "_gathers") else None
        if plan is None:
            if not hasattr(self, "_gathers"):
                self._gathers = {}
            plan = self._gathers[key] = RootGather((self.obs, self.reward, self.done), dst=dst, group=group)
        return plan()


class HistoryTensors:
    """The frame history of a ProcgenVecEnv made with history=dict(...): zero-copy tensors over the ring and its flags."""

    def __init__(self, env, frames=None, gray=False):
        """frames: the tensor the engine was given, or None for a view of the engine's own ring (of 1 plane if `gray`)."""
        L, h, n = env.L, env._h, env.num_envs
        self._env = env
        self.capacity = int(L.pgv_history_capacity(h))
        if frames is None:
            shape = (self.capacity, n, 1 if gray else 3, 64, 64)
            frames = _device_view(L.pgv_history_frames(h), shape[0] * n * shape[2] * 4096, "|u1", env.device).view(shape)
        self.frames = frames  # u8 [T, N, C, 64, 64]
        self.began = _device_view(L.pgv_history_began(h), self.capacity * n, "|u1", env.device).view(self.capacity, n)
        self.pending = _device_view(L.pgv_history_pending(h), n, "|u1", env.device)

    @property
    def head(self):
        """The pushes so far: push p is held while head - capacity <= p < head."""
        return int(self._env.L.pgv_history_head(self._env._h))


class TransitionTensors:
    """The record ring of a ProcgenVecEnv made with transitions=True: zero-copy [T, N] views; row q lives in slot q % T."""

    def __init__(self, env):
        L, h, n = env.L, env._h, env.num_envs
        T = int(L.pgv_history_capacity(h))
        self.capacity = T
        self.action = _device_view(L.pgv_transitions_action(h), T * n, "<i4", env.device).view(T, n)
        self.reward = _device_view(L.pgv_transitions_reward(h), T * n, "<f4", env.device).view(T, n)
        self.flags = _device_view(L.pgv_transitions_flags(h), T * n, "|u1", env.device).view(T, n)


Transition = collections.namedtuple("Transition", "obs next_obs action nstep_return discount steps status")


def _augment_config(augment):
    """The pglib.GatherAug of history_gather's augment= dict; ValueError for anything the engine would refuse, and for more:
    keys it does not know, a missing seed, values of the wrong type."""
    def integer(x):
        return isinstance(x, int) and not isinstance(x, bool)

    if not isinstance(augment, dict):
        raise ValueError("augment must be None or a dict with the keys size, pad, edge, cutout, cutout_color, seed")
    unknown = set(augment) - {"size", "pad", "edge", "cutout", "cutout_color", "seed"}
    if unknown:
        raise ValueError("augment: unknown key(s) %s" % ", ".join(sorted(unknown)))
    if "size" not in augment or "seed" not in augment:
        raise ValueError("augment: size and seed are required")
    size = augment["size"]
    if integer(size):
        size = (size, size)
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(integer(x) for x in size):
        raise ValueError("augment: size must be an integer or a pair (H, W) of integers")
    height, width = size
    if not 1 <= height <= 64:
        raise ValueError("augment: the height must be in 1 .. 64")
    if not 8 <= width <= 64 or width % 8:
        raise ValueError("augment: the width must be in 8 .. 64 and a multiple of 8")
    pad = augment.get("pad", 0)
    if not integer(pad) or not 0 <= pad <= 16:
        raise ValueError("augment: pad must be an integer in 0 .. 16")
    edge = augment.get("edge", "replicate")
    if not isinstance(edge, str) or edge not in pglib.AUG_EDGES:
        raise ValueError("augment: edge must be one of %s" % ", ".join(pglib.AUG_EDGES))
    cutout = augment.get("cutout")
    lo = hi = 0
    if cutout is not None:
        if not isinstance(cutout, (tuple, list)) or len(cutout) != 2 or not all(integer(x) for x in cutout):
            raise ValueError("augment: cutout must be None or a pair (lo, hi) of integers")
        lo, hi = cutout
        if not 1 <= lo <= hi <= 64:
            raise ValueError("augment: cutout needs 1 <= lo <= hi <= 64")
    color = augment.get("cutout_color", "black")
    if not isinstance(color, str) or color not in pglib.AUG_CUTOUT_COLORS:
        raise ValueError("augment: cutout_color must be one of %s" % ", ".join(pglib.AUG_CUTOUT_COLORS))
    seed = augment["seed"]
    if not integer(seed) or not 0 <= seed <= 0xFFFFFFFF:
        raise ValueError("augment: seed must be an integer in 0 .. 2^32 - 1")
    return pglib.gather_aug(height, width, pad, edge, lo, hi, color, seed)


def _history_config(history):
    """(capacity, gray) of ProcgenVecEnv's history= argument, or None; ValueError for anything else."""
    if history is None:
        return None
    if not isinstance(history, dict):
        raise ValueError("history must be None or a dict with the keys capacity, gray")
    unknown = set(history) - {"capacity", "gray"}
    if unknown:
        raise ValueError("history: unknown key(s) %s" % ", ".join(sorted(unknown)))
    capacity, gray = history.get("capacity"), history.get("gray", False)
    if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
        raise ValueError("history: capacity must be an integer >= 1")
    if gray not in (True, False, 0, 1):
        raise ValueError("history: gray must be True or False")
    return capacity, bool(gray)


def _policy_obs_config(policy_obs):
    """(stack, gray, dtype name) of ProcgenVecEnv's policy_obs= argument, or None; ValueError for anything else."""
    if policy_obs is None:
        return None
    if not isinstance(policy_obs, dict):
        raise ValueError("policy_obs must be None or a dict with the keys stack, gray, dtype")
    unknown = set(policy_obs) - {"stack", "gray", "dtype"}
    if unknown:
        raise ValueError("policy_obs: unknown key(s) %s" % ", ".join(sorted(unknown)))
    stack, gray, dtype = policy_obs.get("stack", 4), policy_obs.get("gray", True), policy_obs.get("dtype", "float16")
    if isinstance(stack, bool) or not isinstance(stack, int) or not 1 <= stack <= 8:
        raise ValueError("policy_obs: stack must be an integer in 1 .. 8")
    if gray not in (True, False, 0, 1):
        raise ValueError("policy_obs: gray must be True or False")
    if isinstance(dtype, torch.dtype):
        dtype = str(dtype).replace("torch.", "")
    if dtype not in pglib.POLICY_DTYPES:
        raise ValueError("policy_obs: dtype must be one of %s" % ", ".join(pglib.POLICY_DTYPES))
    return int(stack), bool(gray), dtype


class _DeviceArray:
    """A block of the engine's device memory as `__cuda_array_interface__` describes one (torch.as_tensor wraps it
    without a copy)."""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (int(ptr), False), "version": 2,
                                         "strides": None}


def _device_view(ptr, count, typestr, device):
    if not ptr:
        raise pglib.EngineError("the engine returned a NULL device pointer")
    return torch.as_tensor(_DeviceArray(ptr, count, typestr), device=device)


class EpisodeTensors:
    """Zero-copy tensors over the engine's episode outputs (include/procgen2_vec.h pgv_episode_outputs), written by every
    step_episodes and valid until the next: reward f32[N], terminated / truncated / ended u8[N], counts int32[2] (episodes
    that ended in the step; how many of them have a row in final_obs), ended_env int32[N] (ascending), ended_return f32[N],
    ended_length int32[N], ended_level uint32[N], ended_level_known u8[N] (all parallel to ended_env, meaningful up to
    counts[0]), final_obs u8[capacity, 64, 64, 3] (rows up to counts[1]), and the writable running_return f32[N] /
    running_length int32[N] of the episode each env is in."""

    def __init__(self, out, n, capacity, device):
        for name, typestr in (("reward", "<f4"), ("terminated", "|u1"), ("truncated", "|u1"), ("ended", "|u1"), ("ended_env", "<i4"),
                              ("ended_return", "<f4"), ("ended_length", "<i4"), ("ended_level", "<u4"), ("ended_level_known", "|u1"),
                              ("running_return", "<f4"), ("running_length", "<i4")):
            setattr(self, name, _device_view(getattr(out, name), n, typestr, device))
        self.counts = _device_view(out.counts, 2, "<i4", device)
        self.capacity = capacity
        if capacity:
            self.final_obs = _device_view(out.final_obs, capacity * pglib.OBS_BYTES, "|u1", device).view(capacity, 64, 64, 3)
        else:
            self.final_obs = torch.zeros((0, 64, 64, 3), dtype=torch.uint8, device=device)


class SequenceResult:
    """What ProcgenVecEnv.step_sequence returns (and takes as `out`): obs, rewards f32 [T, N], dones u8 [T, N], seq_return
    f32 [N], seq_length i32 [N], seq_done u8 [N]; a part that was not asked for is None."""

    def __init__(self, rewards=None, dones=None, seq_return=None, seq_length=None, seq_done=None, obs=None):
        self.obs, self.rewards, self.dones = obs, rewards, dones
        self.seq_return, self.seq_length, self.seq_done = seq_return, seq_length, seq_done

    @staticmethod
    def layout(T, n):
        return {"rewards": ((T, n), torch.float32), "dones": ((T, n), torch.uint8), "seq_return": ((n,), torch.float32),
                "seq_length": ((n,), torch.int32), "seq_done": ((n,), torch.uint8)}


# What ProcgenVecEnv.get_levels returns and set_levels takes: tiles uint8 [B, cells], agent_cell / goal_cell int32 [B],
# background int32 [B], background_shift float32 [B].  The tensors are edited in place; _replace(...) swaps one for another.
Levels = collections.namedtuple("Levels", "tiles agent_cell goal_cell background background_shift")


class TilePaths:
    """What ProcgenVecEnv.tile_paths returns: dist int16 [B, cells] or None, probe_dist int32 [B], probe_step uint8 [B],
    cells int32 [B, 2] (source cell, probe cell)."""

    def __init__(self, dist, probe_dist, probe_step, cells):
        self.dist, self.probe_dist, self.probe_step, self.cells = dist, probe_dist, probe_step, cells


class EnvRecords:
    """State records of K envs (ProcgenVecEnv.save_envs): `data`, uint8 [K, record_bytes] on the env's device, and `tag`,
    the fingerprint of the configuration they belong to.  records[i] — an int, a slice, a tensor of indices or a mask —
    is the EnvRecords of that selection (a view where torch gives one) and keeps the tag."""

    def __init__(self, data, tag):
        self.data, self.tag = data, int(tag)

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, item):
        if isinstance(item, int):
            item = slice(item, item + 1) if item != -1 else slice(item, None)
        return EnvRecords(self.data[item], self.tag)

    def clone(self):
        return EnvRecords(self.data.clone(), self.tag)


def step_many_synthetic(envs, steps, run_seed=0):
    """`steps` synthetic steps of several ProcgenVecEnv on one device side by side, each on its own stream, with no
    ordering against the caller's stream and no host work between the launches (include/procgen2_vec.h
    pgv_step_synthetic_many).  Call sync() on the envs before reading their outputs."""
    handles = (c_void_p * len(envs))(*[e._h for e in envs])
    pglib.check(envs[0].L, envs[0].L.pgv_step_synthetic_many(handles, len(envs), int(steps), int(run_seed)),
                "pgv_step_synthetic_many")


def step_phases_many(envs, steps, run_seed=0):
    """`steps` synthetic steps of several ProcgenVecEnv side by side (as step_many_synthetic), every step of every env cut
    into its phases by HIP events on that env's stream (pgv_step_phases_many): numpy float32 [len(envs), 5, steps] —
    step, logic, prepass, render, late, milliseconds."""
    import numpy as np
    out = np.zeros((len(envs), 5, int(steps)), np.float32)
    handles = (c_void_p * len(envs))(*[e._h for e in envs])
    pglib.check(envs[0].L, envs[0].L.pgv_step_phases_many(handles, len(envs), int(steps), int(run_seed), c_void_p(out.ctypes.data)),
                "pgv_step_phases_many")
    return out


class RootGather:
    """Rooted gather of a tuple of per-rank tensors `[n_r, ...]` into `[sum n_r, ...]` slabs on rank `dst` of `group`
    (SURVEY.md §8e).  Ranks may hold different env counts.

    Built once: the counts are exchanged once (one all_gather of an int per rank) and the root allocates one slab per
    tensor.  Every call is one `batch_isend_irecv`: the root receives each peer's block STRAIGHT into its slice of the
    slab (no temporaries, no concatenation) while copying its own block, every peer sends its tensors as they are.  On
    GPUs this is RCCL grouped send/recv, so the root's inbound xGMI links (one per peer, point to point) all run at
    once; the CPU tests run the same code over gloo.  The returned slabs are reused by the next call."""

    def __init__(self, tensors, dst=0, group=None, slabs=None):
        """slabs: the root's preallocated `[sum n_r, ...]` tensors (one per input).  When the root's own input IS its
        slice of the slab (the engine writes straight into it), its block is not copied."""
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.tensors = tuple(tensors)
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)  # rank inside `group`, like dst
        self.dst = dst
        # P2P ops address peers by GLOBAL rank.
        self.global_rank = [dist.get_global_rank(group, r) if group is not None else r for r in range(self.world)]
        n = self.tensors[0].shape[0]
        counts = [None] * self.world
        dist.all_gather_object(counts, int(n), group=group)  # once, on the host: no device sync per call later
        self.counts = [int(c) for c in counts]
        self.offsets = [0]
        for c in self.counts:
            self.offsets.append(self.offsets[-1] + c)
        self.slabs = None
        if self.rank == dst:
            total = self.offsets[-1]
            if slabs is not None:
                self.slabs = tuple(slabs)
                for t, slab in zip(self.tensors, self.slabs):
                    if (tuple(slab.shape) != (total,) + tuple(t.shape[1:]) or slab.dtype != t.dtype or slab.device != t.device
                            or not slab.is_contiguous()):
                        raise ValueError("RootGather: a slab does not match [%d, ...] of its tensor (shape, dtype, device, "
                                         "contiguity)" % total)
            else:
                self.slabs = tuple(torch.empty((total,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
                                   for t in self.tensors)

    def __call__(self):
        dist = self.dist
        ops = []
        if self.rank == self.dst:
            for t, slab in zip(self.tensors, self.slabs):
                for r in range(self.world):
                    part = slab[self.offsets[r]:self.offsets[r + 1]]  # contiguous: a block of leading indices
                    if r == self.rank:
                        if part.data_ptr() != t.data_ptr():  # (already in place when the input is the slab's slice)
                            part.copy_(t)
                    elif self.counts[r]:
                        ops.append(dist.P2POp(dist.irecv, part, self.global_rank[r], group=self.group))
        elif self.counts[self.rank]:
            for t in self.tensors:
                ops.append(dist.P2POp(dist.isend, t.contiguous(), self.global_rank[self.dst], group=self.group))
        if ops:
            for q in dist.batch_isend_irecv(ops):
                q.wait()
        return self.slabs if self.rank == self.dst else tuple(None for _ in self.tensors)


def gather_outputs(obs, reward, done, dst=0, group=None):
    """One-shot form of RootGather (builds the plan, runs it once)."""
    return RootGather((obs, reward, done), dst=dst, group=group)()
