/* rainbow_hip.h — C ABI of librainbow_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the Rainbow *learn step* hot path of
 * Kaixhin/Rainbow (reference = /root/reference, Python only, no FFI of its own).
 * The reference's boundary is the Python class surface consumed by main.py/test.py
 * (SURVEY.md §8b); rainbow_amd/{memory,agent}.py keep that surface and forward to the
 * entry points below through ctypes.  Every entry point cites the reference code it
 * replaces as  file:line  relative to /root/reference.
 *
 * Conventions
 *   - plain C types only; no torch types cross this boundary;
 *   - every pointer named *_dev is a DEVICE pointer (HBM); *_host is host memory;
 *   - every call returns 0 on success, <0 on error (rb_last_error() has the text);
 *     nothing throws across the ABI;
 *   - every launch takes an explicit stream (a hipStream_t passed as void*);
 *     calls are asynchronous unless stated otherwise;
 *   - replay/tree/activation memory is OWNED by the library; parameter, gradient and
 *     noise memory is BORROWED from the caller (torch tensors' data_ptr());
 *   - handles are thread-compatible, not thread-safe (one handle per host thread).
 */
#ifndef RAINBOW_HIP_H_
#define RAINBOW_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB_OK 0
#define RB_ERR_INVALID (-1)
#define RB_ERR_HIP (-2)
#define RB_ERR_OOM (-3)
#define RB_ERR_STATE (-4)

#define RB_FRAME_H 84
#define RB_FRAME_W 84
#define RB_FRAME_BYTES (84 * 84) /* memory.py:7 'state' u8[84,84] */

typedef void* rb_stream_t; /* hipStream_t */
/* Opaque description of a pending noise resample (rb_learner_noise_job) that another launch of the
 * library can host as extra workgroups (rb_replay_sample_fused_noise).                       */
typedef struct { uint64_t opaque[32]; } rb_noise_job_t;
typedef struct rb_replay rb_replay_t;
typedef struct rb_learner rb_learner_t;

const char* rb_last_error(void);
int rb_abi_version(void);
/* Hash of the sources this binary was built from (__graft_entry__.source_hash(), baked in at build time; "" for a build
 * made by hand).  bench.py and smoke() print it, build() rebuilds when it differs from the sources in the tree.        */
const char* rb_source_hash(void);
/* Synchronous copies between host memory and library/torch-owned device memory (state
 * dump/restore of the replay buffer — main.py:94-100,118 pickles the whole memory — and
 * white-box tests).  `stream` is synchronised first.                                     */
int rb_copy_to_host(void* dst_host, const void* src_dev, size_t nbytes, rb_stream_t stream);
int rb_copy_to_device(void* dst_dev, const void* src_host, size_t nbytes, rb_stream_t stream);

/* Live kernel timing for bench.py's roofline line: every launch whose kernel expression
 * contains `kernel_substr` (e.g. "FcHFwdProb") is bracketed by two hipEvents recorded on the
 * stream it is launched on.  NULL/"" disables.  Not for use under stream capture.
 * rb_profile_read synchronises the recorded events, returns their summed elapsed time and
 * the number of launches, and resets the counters.                                        */
int rb_profile_select(const char* kernel_substr);
/* Bracket only every `every`-th matching launch (default 1 = all): an event pair costs the stream ~5 us, so a timed
 * region that samples 1 launch in 8 is perturbed by 0.6 us per step instead of 5.                                    */
int rb_profile_stride(int32_t every);
int rb_profile_read(double* total_ms, int64_t* launches);
/* Cost of an event pair with NOTHING between them on `stream` (mean of n pairs, ms): what the
 * bracketing itself adds to every rb_profile_read sample.  Blocks until the stream drains.     */
int rb_profile_overhead(rb_stream_t stream, int32_t n, double* mean_ms);
/* Test hook (no reference counterpart).  With RB_GUARD=1 in the environment when the library is loaded, every device
 * allocation the library owns (replay ring, sum-tree, learner workspaces) sits between two 4 KiB guard bands; this call
 * synchronises the device and reports how many blocks are live and how many have a band that a kernel wrote into
 * (tests/test_guard.py).  Under RB_GUARD=1 the block between the bands is zeroed; RB_GUARD=2 is the same in every other
 * respect but leaves the block at the bands' fill byte 0xC5 (as f32 a finite -6.3e3, as an integer nonsense), so that a
 * kernel reading memory nobody has written changes its result: the same run under 1 and under 2 must give bit-identical
 * outputs (tests/test_poison_emu.py, tests/test_poison_gpu.py).  Without RB_GUARD it reports 0 / 0.                  */
int rb_debug_check_guards(int64_t* n_blocks, int64_t* n_bad);

/* ===================================================================== replay ==
 * HBM-resident prioritised replay: SoA ring (frames u8[C][7056], timestep i32[C],
 * action i32[C], reward f32[C], nonterminal u8[C]) + level-order float32 sum-tree
 * with the reference's truncated leaf level (memory.py:17-18).                  */

/* Device-resident header; host reads it with rb_replay_header (synchronising).   */
typedef struct {
  int64_t index;   /* SegmentTree.index   memory.py:14,59 */
  int32_t full;    /* SegmentTree.full    memory.py:16,60 */
  float max;       /* SegmentTree.max     memory.py:20,48,54,61 (p^w domain) */
  float total;     /* sum_tree[0]         memory.py:88-89 */
  int32_t last_attempts; /* sampler attempts used by the last rb_replay_sample */
  int32_t last_status;   /* 0 ok, 1 = gave up after max attempts */
  uint64_t rng_counter;  /* Philox counter of the device sampler */
} rb_replay_header_t;

/* Raw device pointers, for state dump/restore and white-box tests.               */
typedef struct {
  float* sum_tree_dev;    int64_t tree_len;   /* tree_start + capacity */
  int64_t tree_start;
  uint8_t* frames_dev;    /* [capacity][7056] */
  int32_t* timestep_dev;  int32_t* action_dev;
  float* reward_dev;      uint8_t* nonterminal_dev;
  rb_replay_header_t* header_dev;
  int32_t* window_dev;    /* [max_batch][history+multi_step] ring index of every window slot of the last sample */
  int32_t window_len;
} rb_replay_buffers_t;

/* ReplayMemory.__init__ + SegmentTree.__init__  (memory.py:92-102, 13-20).
 * capacity must be even and >= 2 (odd capacities crash the reference). */
int rb_replay_create(rb_replay_t** out, int64_t capacity, int32_t history, int32_t multi_step,
                     double discount, double priority_exponent, uint64_t seed);
/* The same replay holding S interleaved environment streams (1 <= S <= 64; S = 1 is rb_replay_create's replay): one ring, one
 * sum tree, stream s owns the slots s, s + S, s + 2S, ...  Windows, n-step returns, the validity test of the sampler and the
 * validation stacks follow the stream's own slots (stride S); IS weights count every stored transition (memory.py:152).
 * Refused with RB_ERR_INVALID and a message: S outside [1, 64], capacity not a multiple of S, capacity <= (history +
 * multi_step) * S.  Such a replay is filled by whole rounds (rb_replay_append_streams, or rb_replay_append_batch with a
 * multiple of S transitions already in ring order); rb_replay_append refuses it.                                         */
int rb_replay_create_streams(rb_replay_t** out, int64_t capacity, int32_t history, int32_t multi_step, double discount,
                             double priority_exponent, uint64_t seed, int32_t streams);
/* The stream count S of a replay (1 for rb_replay_create's). */
int rb_replay_streams(rb_replay_t* r, int32_t* streams_host);
int rb_replay_destroy(rb_replay_t* r);
int rb_replay_buffers(rb_replay_t* r, rb_replay_buffers_t* out_host);
/* synchronises `stream`, then copies the header to host */
int rb_replay_header(rb_replay_t* r, rb_replay_header_t* out_host, rb_stream_t stream);

/* Frame preprocessing of the environment wrapper on the device (env.py:27-29 `_get_state` =
 * cv2.resize(ale.getScreenGrayscale() u8 [height][width], (84, 84), INTER_LINEAR) as float32 / 255, and env.py:57-69: the
 * observation of a step is the element-wise max of the states after frames 3 and 4 of the action repeat).
 * frame_a_dev / frame_b_dev: n raw grayscale screens each ([n][height][width] u8; frame_b_dev NULL = no max, env.py:50 reset);
 * out_dev: [n][84][84] float32 in [0, 1] — one slice of the `state` tensor that Agent.act and ReplayMemory.append take.
 * PARITY UNPINNED: cv2 is absent from the build container; the kernel is bit-exact against oracle/frame_oracle.py, a
 * restatement of OpenCV's published 8-bit fixed-point INTER_LINEAR (11-bit coefficients).                                  */
int rb_frame_preprocess(const uint8_t* frame_a_dev, const uint8_t* frame_b_dev, int32_t height, int32_t width, int32_t n,
                        float* out_dev, rb_stream_t stream);

/* The observation front end of S host emulators (env.py's wrapper around ALE) for all S streams in ONE launch per round:
 * the resize and frame max of rb_frame_preprocess plus the state deque (env.py:24,68,77), its blanking at a true reset
 * (env.py:31-33,41), the life-loss reset that must not blank (env.py:36-38,49-52) and the truncated action repeat
 * (env.py:56-67: a frame of the pair that was never taken stays zero).  Stateless, like rb_frame_preprocess.
 * frames_a_dev / frames_b_dev: u8 [streams][height][width] each (the screens after frames 3 and 4 of the repeat); either may
 * be NULL when no stream's flags name it.  stacks_in_dev / stacks_out_dev: f32 [streams][history][84][84], oldest frame first,
 * 16-byte aligned, out of place (they must not overlap) — the layout rb_learner_act_batch and rb_replay_append_streams* take.
 * flags_host: `streams` bytes of host memory, passed to the kernel by value (reusable when the call returns); per stream a
 * bit set of RB_OBS_*.  All eight values are defined:
 *  - frames 0 .. history-2 of the output are frames 1 .. history-1 of the input, or all zeros if RB_OBS_BLANK is set;
 *  - frame history-1 of the output is the element-wise max over the PRESENT frames (RB_OBS_FRAME_A, RB_OBS_FRAME_B) of
 *    resize(frame) / 255 — bit-identical to rb_frame_preprocess on the same screens — or zeros if neither is present.
 * What each value stands for in env.py:
 *    FRAME_A | FRAME_B (6)   step(), the whole repeat ran (env.py:58-68)
 *    BLANK | FRAME_A   (3)   reset() of a new game (env.py:40-52)
 *    FRAME_A           (2)   reset() after a lost life: one no-op, no blanking (env.py:36-38,49-52); also step() whose
 *                            repeat was cut after its third frame (env.py:60-61,65-66)
 *    0                       step() whose repeat was cut before its third frame (env.py:56,65-67: both frames zero)
 * Refused with RB_ERR_INVALID and a message that names the argument: NULL or misaligned or overlapping stacks, NULL
 * flags_host, streams outside [1, 64], history outside [1, 16], height or width outside [2, 4096], a flag byte above 7, a
 * flag that names a frame whose pointer is NULL.  Same PARITY UNPINNED caveat as rb_frame_preprocess.                       */
#define RB_OBS_BLANK 1
#define RB_OBS_FRAME_A 2
#define RB_OBS_FRAME_B 4
int rb_obs_stack_step(const uint8_t* frames_a_dev, const uint8_t* frames_b_dev, int32_t height, int32_t width, int32_t streams,
                      int32_t history, const uint8_t* flags_host, const float* stacks_in_dev, float* stacks_out_dev,
                      rb_stream_t stream);

/* ReplayMemory.append (memory.py:105-108) + SegmentTree.append (memory.py:56-61):
 * quantises state_dev[history-1] (f32 in [0,1]) to u8 by x*255 truncation ON DEVICE,
 * stores (timestep, frame, action, reward, nonterminal) at `index`, sets the leaf to
 * the running max priority and walks the sums to the root.                        */
int rb_replay_append(rb_replay_t* r, const float* state_dev, int32_t timestep, int32_t action,
                     float reward, int32_t nonterminal, rb_stream_t stream);
/* n sequential appends of already-quantised frames (same result as n calls of
 * rb_replay_append: all leaves get the current max, memory.py:107).               */
int rb_replay_append_batch(rb_replay_t* r, const uint8_t* frames_dev, const int32_t* timesteps_dev,
                           const int32_t* actions_dev, const float* rewards_dev,
                           const uint8_t* nonterminals_dev, int64_t n, rb_stream_t stream);

/* One append ROUND of an S-stream replay: ReplayMemory.append (memory.py:105-108) for streams 0 .. S-1 in that order, in ONE
 * launch.  states_dev: f32 [S][history][84][84] (16-byte aligned; what rb_learner_act_batch just consumed), state[s][history-1]
 * quantised as rb_replay_append does.  timesteps_host, actions_host, rewards_host, nonterminals_host: S values each, host
 * memory, passed to the kernel by value — asynchronous, and the arrays may be reused as soon as the call returns.  Ring,
 * tree and header end bit-identical to S sequential appends.  The write head must be at a round boundary (a multiple of S). */
int rb_replay_append_streams(rb_replay_t* r, const float* states_dev, const int32_t* timesteps_host, const int32_t* actions_host,
                             const float* rewards_host, const uint8_t* nonterminals_host, rb_stream_t stream);

/* The same round with DEVICE operands, for a round that never leaves the device (actions from rb_learner_act_batch, rewards and
 * nonterminals from a device environment such as rb_catch_step): timesteps_dev i32[S], actions_dev i32[S], rewards_dev f32[S],
 * nonterminals_dev u8[S].  timesteps_dev is IN/OUT: the kernel stores the value it read and writes back
 * `nonterminal ? t + 1 : 0` (memory.py:108 per stream), so the caller keeps no host copy of the episode timesteps.  The
 * arrays are read when the launch runs (stream order), not at the call.  Same refusals as rb_replay_append_streams; ring, tree
 * and header end bit-identical to the host-operand call with the same values.                                                */
int rb_replay_append_streams_dev(rb_replay_t* r, const float* states_dev, int32_t* timesteps_dev, const int32_t* actions_dev,
                                 const float* rewards_dev, const uint8_t* nonterminals_dev, rb_stream_t stream);

/* ================================================================ device Catch ==
 * A small built-in environment that lives on the device: S independent games of Catch on the 84 x 84 screen, one workgroup
 * per stream, so that a training round (act -> step -> append) is launches on one stream with no synchronisation.
 * Rules:
 *  - logical grid 12 x 12, one cell = 7 x 7 pixels; the ball is 1 cell at intensity 1.0, the paddle 3 cells wide on the
 *    bottom row (row 11) at intensity 0.5, background 0 (255, 127 and 0 after the replay's x * 255 truncation);
 *  - actions: 0 stay, 1 left, 2 right (the paddle's left cell moves by one, clamped to [0, 9]); 3 actions; any other value
 *    counts as stay;
 *  - per step the paddle moves, then the ball falls one row; when the ball reaches the bottom row the episode ends with
 *    reward +1 if its column lies under the paddle, else -1; every other step has reward 0 (an episode is 11 steps);
 *  - episode e (0, 1, 2, ...) of stream s starts with the ball in row 0, column x0 % 12, and the paddle's left cell at
 *    x1 % 10, where (x0, x1, ., .) = Philox4x32-10(key = seed, counter = (lo = e, hi = s)): counter-based, no stored
 *    generator state.  rb_catch_reset starts the NEXT episode of every stream (the first call starts episode 0);
 *  - the observation of a state is the rendered 84 x 84 frame; a frame stack is f32 [history][84][84], oldest first.
 * stacks_* are f32 [S][history][84][84], 16-byte aligned: the layout rb_learner_act_batch and rb_replay_append_streams* take. */
typedef struct rb_catch rb_catch_t;
typedef struct {
  int64_t episodes;     /* episodes finished since create / rb_catch_reset_stats, all streams */
  int64_t catches;      /* of which the ball was caught */
  double return_sum;    /* sum of the episode returns */
} rb_catch_stats_t;
#define RB_CATCH_ACTIONS 3
/* 1 <= streams <= 64, 1 <= history <= 16. */
int rb_catch_create(rb_catch_t** out, int32_t streams, int32_t history, uint64_t seed);
int rb_catch_destroy(rb_catch_t* c);
/* Every stream starts its next episode; stacks_dev gets the S reset stacks (history - 1 zero frames, then the first
 * observation: env.py:44-52).  Asynchronous.                                                                      */
int rb_catch_reset(rb_catch_t* c, float* stacks_dev, rb_stream_t stream);
/* One step of every stream (one launch, asynchronous): actions_dev i32[S] in; rewards_dev f32[S], nonterminals_dev u8[S]
 * (0 = this step ended the episode) out.  stacks_out[s] = stacks_in[s] shifted by one frame with the new observation last
 * (env.py:70); where the step ended the episode, stacks_out[s] is instead the reset stack of the stream's next episode (what
 * main.py:147-148 hands to the next act).  Out of place: stacks_out_dev must not overlap stacks_in_dev.  Needs a
 * rb_catch_reset first (RB_ERR_STATE otherwise).                                                                          */
int rb_catch_step(rb_catch_t* c, const int32_t* actions_dev, const float* stacks_in_dev, float* stacks_out_dev,
                  float* rewards_dev, uint8_t* nonterminals_dev, rb_stream_t stream);
/* Totals the device has accumulated (a training loop never has to synchronise to know how it is doing).  SYNCHRONISES `stream`. */
int rb_catch_stats(rb_catch_t* c, rb_catch_stats_t* out_host, rb_stream_t stream);
/* Zero those totals (stream-ordered, asynchronous). */
int rb_catch_reset_stats(rb_catch_t* c, rb_stream_t stream);

/* ============================================================= device Breakout ==
 * A second built-in environment on the device, with what Catch lacks: lives (a lost life is a terminal for training while the
 * game goes on, env.py:70-75), episodes of varying length, rewards inside an episode and rewards above 1 (so that reward
 * clipping, main.py:155-156, matters).  S independent games, one workgroup per stream, the same buffers as device Catch.
 * Rules (all integer):
 *  - logical grid 12 x 12, one cell = 7 x 7 pixels.  Ball: 1 cell at intensity 1.0; bricks: rows 1, 2, 3, 36 of them, at 0.75;
 *    paddle: 2 cells wide on row 11 at 0.5, its left cell p in [0, 10]; background 0 (255, 191, 127 and 0 after the replay's
 *    x * 255 truncation).  Row r keeps a 12-bit mask, bit c = column c.  The ball is at (bx, by), by in [0, 10], and moves
 *    by (dx, dy), both in {-1, +1}.  It is never on a brick cell.  3 lives per game; t counts the steps of the game in play;
 *    max_steps ends a game as ALE's max_num_frames_per_episode does;
 *  - serve k (0, 1, 2, ...; per stream, 0xFFFFFFFF before the first reset) of stream s: (x0, x1, x2, .) = Philox4x32-10(key =
 *    seed, counter = (lo = k, hi = s)), the generator of device Catch; bx = x0 % 12, by = 4, dx = (x1 & 1) ? +1 : -1, dy = +1;
 *  - a new game is a serve that also sets p = x2 % 11, refills all bricks, sets lives = 3 and t = 0;
 *  - one step with action a (0 stay, 1 left, 2 right; 3 actions; any other value counts as stay), in this order:
 *      1. a == 1: p = max(p - 1, 0);  a == 2: p = min(p + 1, 10)
 *      2. t += 1; reward = 0; lost = over = false
 *      3. nx = bx + dx; if nx < 0 or nx > 11: dx = -dx, nx = bx + dx
 *         ny = by + dy; if ny < 0:            dy = +1,  ny = by + dy
 *      4. if 1 <= ny <= 3 and brick (ny, nx) stands: remove it, reward = 5 - ny, dy = -dy (the ball does not move this step)
 *         else if ny == 11:
 *              if p <= nx <= p + 1: bx = nx, dy = -1, dx = (nx == p) ? -1 : +1 (by stays 10); if no brick is left: refill all 36
 *              else:                lives -= 1, lost = true, over = (lives == 0)
 *         else: bx = nx, by = ny
 *      5. if t == max_steps: over = true
 *      6. if over: new game (k += 1); else if lost: serve (k += 1; bricks, paddle, lives and t stay)
 *    Bricks pay 2 / 3 / 4 in rows 3 / 2 / 1;
 *  - outputs of a step: reward f32 (0, 2, 3 or 4); nonterminal 0 where over, and with life_terminals != 0 also where lost, else
 *    1; stacks_out[s] = where over, the reset stack of the new game (history - 1 zero frames, then its first observation,
 *    env.py:40-52), otherwise stacks_in[s] shifted by one frame with the render of the NEW state last — after a lost life that
 *    is the serve state: the stack moves one frame per round and is not blanked (the convention of the host emulators' loop);
 *  - totals per stream: steps, bricks hit, lives lost, games finished, and return_sum = the sum of the returns (all rewards of
 *    a game, unclipped) of the games FINISHED; game_return is the return so far of the game in play.                       */
typedef struct rb_breakout rb_breakout_t;
/* The whole state of one stream, 64 bytes, the device's own layout (exact checkpoints, and states random play never reaches). */
typedef struct {
  int32_t bx, by;       /* ball cell: column in [0, 11], row in [0, 10] */
  int32_t dx, dy;       /* -1 or +1 each */
  int32_t paddle;       /* left cell, in [0, 10] */
  int32_t t;            /* steps of the game in play, in [0, max_steps) */
  uint32_t k;           /* number of the last serve (0xFFFFFFFF: none yet) */
  uint16_t rows[3];     /* bricks of rows 1, 2, 3: bit c = column c */
  uint16_t lives;       /* in [1, 3] */
  int32_t game_return;  /* rewards of the game in play */
  int32_t games, return_sum, bricks, lives_lost, steps;   /* totals since create / rb_breakout_reset_stats, all >= 0 */
  int32_t reserved;     /* 0 */
} rb_breakout_state_t;
typedef struct {
  int64_t games;        /* games finished since create / rb_breakout_reset_stats, all streams */
  double return_sum;    /* sum of their returns (unclipped) */
  int64_t bricks;       /* bricks hit */
  int64_t lives_lost;
  int64_t steps;
} rb_breakout_stats_t;
#define RB_BREAKOUT_ACTIONS 3
/* 1 <= streams <= 64, 1 <= history <= 16, 1 <= max_steps <= 65535. */
int rb_breakout_create(rb_breakout_t** out, int32_t streams, int32_t history, int32_t max_steps, uint64_t seed);
int rb_breakout_destroy(rb_breakout_t* c);
/* Every stream starts its next game (the first call serves k = 0); the game in play is abandoned and counts nothing.
 * stacks_dev gets the S reset stacks.  Asynchronous.                                                                       */
int rb_breakout_reset(rb_breakout_t* c, float* stacks_dev, rb_stream_t stream);
/* One step of every stream (one launch, asynchronous), operands as rb_catch_step's; life_terminals != 0 (training) reports a
 * lost life as nonterminal 0.  Same refusals as rb_catch_step: NULL or misaligned operands, stacks_out_dev overlapping
 * stacks_in_dev, no rb_breakout_reset or rb_breakout_set_state before it (RB_ERR_STATE).                                    */
int rb_breakout_step(rb_breakout_t* c, const int32_t* actions_dev, const float* stacks_in_dev, float* stacks_out_dev,
                     float* rewards_dev, uint8_t* nonterminals_dev, int32_t life_terminals, rb_stream_t stream);
/* The totals, summed over the streams.  SYNCHRONISES `stream`. */
int rb_breakout_stats(rb_breakout_t* c, rb_breakout_stats_t* out_host, rb_stream_t stream);
/* Zero the totals (game_return stays: the game in play goes on).  Stream-ordered, asynchronous. */
int rb_breakout_reset_stats(rb_breakout_t* c, rb_stream_t stream);
/* The states of all S streams to host memory.  SYNCHRONISES `stream`. */
int rb_breakout_get_state(rb_breakout_t* c, rb_breakout_state_t* out_host, rb_stream_t stream);
/* Replace the states of all S streams.  Every field of every stream is validated first (the ranges above, t < max_steps, rows
 * below 4096, the ball not on a brick cell, totals and game_return >= 0, reserved 0): RB_ERR_INVALID names the stream and the
 * field, and nothing is changed.  Marks the handle as reset; the frame stacks are the caller's to restore.  SYNCHRONISES
 * `stream`.                                                                                                             */
int rb_breakout_set_state(rb_breakout_t* c, const rb_breakout_state_t* in_host, rb_stream_t stream);

/* ================================================================ episode tally ==
 * An environment-independent recorder of per-episode returns on the device (test.py:19-41 keeps the list T_rewards): fed with
 * the rewards / nonterminals vectors every round already produces, so that an evaluation round on a device environment
 * (act -> step -> tally) is launches on one stream with no synchronisation, like a training round.  Rewards are taken as they
 * come: evaluation does not clip (test.py:28).
 * Rules:
 *  - S streams share `episodes` slots; stream s has the quota q_s = episodes / S + (s < episodes % S ? 1 : 0) — the quotas sum
 *    to `episodes`, a stream may have quota 0 — so that N episodes are N / S per stream whatever their lengths (counting "the
 *    first N to finish" would over-represent the streams whose episodes are short);
 *  - per stream the tally keeps a running return (f32, ret = ret + r in step order), a running length (i32) and the number of
 *    episodes it has recorded;
 *  - a step adds rewards[s] and 1 to the running values of every stream; where nonterminals[s] == 0 the episode is recorded as
 *    (return, length) if the stream is still under its quota, and the running values are zeroed either way: the reward of the
 *    ending step belongs to the ending episode, episodes that finish after the quota is filled are ignored;
 *  - remaining = sum over s of (q_s - recorded_s); 0 = all `episodes` slots are filled, further steps change nothing on record;
 *  - the record is stream-major: the q_0 slots of stream 0 in the order its episodes ended, then stream 1's, and so on.  A slot
 *    not yet filled reads as (return NaN, length 0); streams_host names the owning stream of every slot, filled or not.      */
typedef struct rb_tally rb_tally_t;
/* 1 <= streams <= 64, 1 <= episodes <= 65536.  The tally starts reset.  Synchronises the null stream. */
int rb_tally_create(rb_tally_t** out, int32_t streams, int32_t episodes);
int rb_tally_destroy(rb_tally_t* t);
/* Start over: every slot unfilled, running values zero, remaining = episodes.  Asynchronous, one launch. */
int rb_tally_reset(rb_tally_t* t, rb_stream_t stream);
/* One step of every stream: rewards_dev f32[S], nonterminals_dev u8[S] (0 = this step ended the episode), read when the launch
 * runs (stream order).  Asynchronous, one launch of one wave.                                                          */
int rb_tally_step(rb_tally_t* t, const float* rewards_dev, const uint8_t* nonterminals_dev, rb_stream_t stream);
/* Episodes still to be recorded.  SYNCHRONISES `stream`. */
int rb_tally_remaining(rb_tally_t* t, int32_t* remaining_host, rb_stream_t stream);
/* The record: returns_host f32, lengths_host i32, streams_host i32, [episodes] each, all three required.  SYNCHRONISES `stream`. */
int rb_tally_read(rb_tally_t* t, float* returns_host, int32_t* lengths_host, int32_t* streams_host, rb_stream_t stream);

/* SegmentTree.find (memory.py:64-82): float64 values against float32 nodes.       */
int rb_replay_find(rb_replay_t* r, const double* values_dev, int32_t n, float* probs_dev,
                   int64_t* data_idx_dev, int64_t* tree_idx_dev, rb_stream_t stream);

/* ReplayMemory.sample (memory.py:124-155), entirely on device:
 * stratified draw (+ whole-batch rejection, memory.py:128-132), tree search, window
 * gather with episode-boundary blanking (memory.py:111-121), n-step return, IS weights.
 * unit_uniforms_dev: NULL = device Philox; else [max_attempts][batch] float64 in [0,1)
 *   (parity hook: the reference's np.random.uniform(0,seg) == seg*u, memory.py:129).
 * Outputs (all device, caller-allocated):
 *   tree_idx i64[B]; states/next_states u8[B][history][7056] (NOT yet /255);
 *   actions i64[B]; returns f32[B]; nonterminals f32[B]; weights f32[B].
 * Status lands in the device header (last_attempts/last_status).                   */
int rb_replay_sample(rb_replay_t* r, int32_t batch, double priority_weight,
                     const double* unit_uniforms_dev, int32_t max_attempts,
                     int64_t* tree_idx_dev, uint8_t* states_dev, uint8_t* next_states_dev,
                     int64_t* actions_dev, float* returns_dev, float* nonterminals_dev,
                     float* weights_dev, rb_stream_t stream);

/* rb_replay_sample + the learner's per-step noise resample (model.py:36-40) in ONE launch: the
 * sampler is a single-workgroup latency chain and the noise draw is independent of it, so the
 * noise workgroups ride along and cost no kernel boundary of their own.  noise_job comes from
 * rb_learner_noise_job (device RNG only).                                                    */
int rb_replay_sample_fused_noise(rb_replay_t* r, int32_t batch, double priority_weight,
                                 const double* unit_uniforms_dev, int32_t max_attempts,
                                 int64_t* tree_idx_dev, uint8_t* states_dev, uint8_t* next_states_dev,
                                 int64_t* actions_dev, float* returns_dev, float* nonterminals_dev,
                                 float* weights_dev, const rb_noise_job_t* noise_job, rb_stream_t stream);

/* The reference's sampler retries until a batch is valid (memory.py:128-132); the device sampler is bounded by
 * max_attempts.  When the bound is hit it writes ZERO importance weights (the learn step that consumes the batch then
 * has an exactly zero gradient), sets last_status = 1 in the device header, marks the draw's index buffer (tree_idx = -1
 * everywhere) and increments a pinned host counter.
 * This call reads that counter WITHOUT synchronising: the number of failed sampler launches that have completed so far. */
int rb_replay_failed_samples(rb_replay_t* r, int64_t* count_host);
/* Zero that counter (after the caller has reported the failure and, e.g., appended more transitions).  A learn step that
 * consumed a failed batch left no trace: its priority write-back (rb_replay_update_priorities and the learner's fused
 * sink: by the mark in the index buffer, rb_replay_dropped_updates), the optimiser update and the optimiser's step number
 * (by last_status of the draw the learn call consumes) are all skipped on the device.  Also zeroes the dropped-update count
 * and the expired-wait count (rb_replay_expired_waits: the early draw is allowed again). */
int rb_replay_reset_failed_samples(rb_replay_t* r);
/* A draw that gave up marks its own index buffer (every tree index = -1).  ReplayMemory.update_priorities (memory.py:157-159)
 * — rb_replay_update_priorities, rb_replay_update_sample and the learner's fused sink — drops exactly the write-back whose
 * indices carry that mark and counts it here (pinned host word, read WITHOUT synchronising: completed launches so far).  The
 * write-back of an earlier, valid batch is applied whatever happened to later draws.                                        */
int rb_replay_dropped_updates(rb_replay_t* r, int64_t* count_host);
/* The early draw (RB_OPTS spec_draw=1, off by default: rb_learner_train_step may issue ReplayMemory.update_priorities of call k and
 * ReplayMemory.sample of call k + 1 — agent.py:100 / :63, memory.py:124-159 — on a stream the replay owns) waits across streams with
 * a bound of ~2 ms and fails safe: an expired wait makes the waiting launch do the work itself (the draw) or drop it (the
 * write-back: also counted by rb_replay_dropped_updates), is counted here (pinned host word, read WITHOUT synchronising) and
 * switches the early draw off on this handle until rb_replay_reset_failed_samples.  0 on a healthy device.                      */
int rb_replay_expired_waits(rb_replay_t* r, int64_t* count_host);
/* SegmentTree.index / .full (memory.py:14,16) from the library's host mirror, without touching the device: exact as long
 * as every append went through this handle (a header restored with rb_copy_to_device is picked up as well).        */
int rb_replay_position(rb_replay_t* r, int64_t* index_host, int32_t* full_host);

/* Graph replay support: when set (non-NULL), rb_replay_sample reads -beta (float32, i.e.
 * float32(-priority_weight), memory.py:153) from this DEVICE location instead of its by-value
 * argument, so main.py:161's per-step annealing works under a captured hipGraph.           */
int rb_replay_set_beta_source(rb_replay_t* r, const float* neg_beta_dev);

/* Annealed update horizon and discount (BBF: n from 10 down to 3 and gamma from 0.97 up to 0.997 after every reset) on a LIVE replay,
 * ring and tree untouched.  n_max is the multi_step the handle was created with; 1 <= n_eff <= n_max and 0 < discount <= 1.  From
 * the next draw on, every output is bit for bit what a replay created with multi_step = n_eff and this discount draws from the same
 * ring, tree and uniforms (memory.py:111-145 with n = n_eff: the return over k < n_eff, the nonterminal at idx + n_eff, the next
 * state from window slots [n_eff, n_eff + history), the write-head rule (index - idx) mod capacity > n_eff).
 *   The stride rule: n_max keeps deciding every allocation and the row stride of the window table — rb_replay_buffers_t.window_len
 *     stays history + n_max, and a reader addresses row i at window_dev + i * window_len whatever n_eff is.
 *   The -1 rule: slots [history + n_eff, history + n_max) of every row are written as -1 (the value of a blanked slot), never a
 *     ring index that may straddle the write head.
 * gamma^k (float32 of the double power, memory.py:101) is stored in stream order by a one-workgroup launch on `stream` that receives
 * the table by value: no copy from pageable memory, no synchronisation; a draw already queued on `stream` sees the old table, the
 * next one the new.  Like every entry point that changes the replay it discards an early draw in flight.  The horizon is a host-side
 * value of the handle: a captured graph freezes the one in force at capture, as it freezes every by-value argument.
 * rb_replay_get_horizon reads the host values (n_max and the creation discount until the first set).                            */
int rb_replay_set_horizon(rb_replay_t* r, int32_t n_eff, double discount, rb_stream_t stream);
int rb_replay_get_horizon(rb_replay_t* r, int32_t* n_eff_host, double* discount_host);

/* SegmentTree.update (memory.py:44-48): raw leaf values, duplicates last-write-wins. */
int rb_replay_update_leaves(rb_replay_t* r, const int64_t* tree_idx_dev, const float* values_dev,
                            int32_t n, rb_stream_t stream);
/* ReplayMemory.update_priorities (memory.py:157-159): p = loss^w, then the above.  */
int rb_replay_update_priorities(rb_replay_t* r, const int64_t* tree_idx_dev,
                                const float* losses_dev, int32_t n, rb_stream_t stream);

/* ReplayMemory.update_priorities(idx, loss) of learn step k (agent.py:100, memory.py:157-159) followed by
 * ReplayMemory.sample(batch) of step k + 1 (agent.py:62, memory.py:148-155) as ONE launch of one workgroup: the update's
 * writes to the top of the tree go straight into the LDS copy the search starts from.  Results (tree, header, batch) are
 * bit-identical to rb_replay_update_priorities followed by rb_replay_sample with the same arguments; upd_n above 64 or batch
 * above 256 take exactly those two calls.  states_dev / next_states_dev may be NULL as in rb_replay_sample.                 */
int rb_replay_update_sample(rb_replay_t* r, const int64_t* upd_tree_idx_dev, const float* upd_losses_dev, int32_t upd_n,
                            int32_t batch, double priority_weight, const double* unit_uniforms_dev, int32_t max_attempts,
                            int64_t* tree_idx_dev, uint8_t* states_dev, uint8_t* next_states_dev,
                            int64_t* actions_dev, float* returns_dev, float* nonterminals_dev,
                            float* weights_dev, rb_stream_t stream);

/* Random-shift augmentation (DrQ, DrQ-eps, SPR) where the stacks are built.  The frame stacks of the LAST draw on this handle
 * (rb_replay_sample* / rb_replay_update_sample called with states_dev = next_states_dev = NULL: the draw leaves its window table
 * behind), each stack shifted by (dy, dx) in [-pad, pad] with edge replication — the 84 x 84 stack padded by `pad` pixels of its
 * border and cropped at a random offset:
 *     out[i][w][c][y][x] = frame[clamp(y + dy)][clamp(x + dx)],  clamp onto [0, 83],  w = 0 state / 1 next state,
 * with ONE (dy, dx) for all `history` frames c of a stack and independent ones for the state and the next state of a sample.  A
 * blanked frame stays 7056 zero bytes.  pad = 0 gives exactly the bytes rb_replay_sample writes when it is handed stack pointers.
 *   shifts_in_dev != NULL: the shifts are read from there, int8 [batch][2][2] = [i][w] -> (dy, dx), clamped to [-pad, pad]
 *                          (the parity hook of the tests);
 *   shifts_in_dev == NULL: Philox4x32-10 with key = seed ^ 0x5348494654 (seed: rb_replay_create's) and counter (hi = draw, lo = i):
 *                          words 0, 1 are the state's (dy, dx), words 2, 3 the next state's, each (int)((word * (2 pad + 1)) >> 32)
 *                          - pad.  `draw` is the caller's batch counter (increment it per batch).  The tagged key keeps these
 *                          draws off the sampler's stream (key = seed, counter (rng_counter + attempt, i)); the device header and
 *                          its rng_counter are neither read nor written.
 *   shifts_out_dev != NULL: receives the shifts actually used, same [batch][2][2] layout.
 * states_dev / next_states_dev: u8[batch][history][7056], 16-byte aligned; batch in [1, 1024], pad in [0, 8].  Reads the replay
 * only (it is no mutation and draws nothing); an early draw in flight is joined first, as by every entry point outside a draw.
 * After a draw that gave up (last_status = 1) the windows of that draw are gathered, as rb_replay_sample's own gather does.
 * The validation view (rb_replay_state_at / rb_replay_states_at) is never shifted.                                          */
int rb_replay_gather_shifted(rb_replay_t* r, int32_t batch, int32_t pad, uint64_t draw,
                             const int8_t* shifts_in_dev,   /* NULL: device Philox */
                             uint8_t* states_dev, uint8_t* next_states_dev,
                             int8_t* shifts_out_dev,        /* may be NULL */
                             rb_stream_t stream);

/* ReplayMemory.__next__ (memory.py:167-178): blanked history stack for data index i,
 * as f32 /255, out_dev f32[history][7056].  With S streams: slots i - (history-1-t) S, t = 0..history-1. */
int rb_replay_state_at(rb_replay_t* r, int64_t data_index, float* out_dev, rb_stream_t stream);

/* The same for n data indices in ONE launch (the validation pass of test.py:38-39 walks the whole validation memory):
 * data_index_dev i64[n], each in [0, capacity); out_dev f32[n][history][7056].                                        */
int rb_replay_states_at(rb_replay_t* r, const int64_t* data_index_dev, int32_t n, float* out_dev,
                        rb_stream_t stream);

/* u8 -> f32 x/255 (memory.py:137-138 `.div_(255)`), correctly-rounded division.    */
int rb_u8_to_unit_f32(const uint8_t* src_dev, float* dst_dev, int64_t n, rb_stream_t stream);

/* ==================================================================== learner ==
 * Rainbow network (model.py) + learn step (agent.py:61-100) on flat f32 buffers.  */

typedef struct {
  int32_t batch;        /* args.batch_size      agent.py:20 */
  int32_t atoms;        /* args.atoms           agent.py:15 */
  int32_t actions;      /* env.action_space()   agent.py:14 */
  int32_t history;      /* args.history_length  model.py:56 */
  int32_t hidden;       /* args.hidden_size     model.py:64 */
  int32_t architecture; /* 0 canonical, 1 data-efficient  model.py:55-63 */
  int32_t multi_step;   /* args.multi_step      agent.py:21 */
  float v_min, v_max;   /* agent.py:16-17 */
  double discount;      /* agent.py:22 */
} rb_learner_config_t;

/* One named tensor inside the flat parameter/gradient buffer (state-dict names of
 * model.py: convs.{0,2,4}.{weight,bias}, fc_*.{weight,bias}_{mu,sigma}).          */
typedef struct {
  char name[48];
  int64_t offset; /* in floats */
  int32_t ndim;
  int32_t shape[4];
} rb_tensor_desc_t;

/* Sizes of the flat buffers (in floats) for a config.                              */
int rb_learner_sizes(const rb_learner_config_t* cfg, int64_t* n_params, int64_t* n_noise);
/* Fills descs[0..*n) ; pass descs=NULL to query the count.                         */
int rb_learner_param_layout(const rb_learner_config_t* cfg, rb_tensor_desc_t* descs, int32_t* n);
/* Noise buffer layout: factorised vectors f(eps) (model.py:32-40), per layer
 * {name = fc_h_v.eps_in, fc_h_v.eps_out, ...}.                                      */
int rb_learner_noise_layout(const rb_learner_config_t* cfg, rb_tensor_desc_t* descs, int32_t* n);
/* Debug read-out (stateless: allocates nothing, touches no device): which kernel every launch of a learn step reaches for this
 * config, with its grid, block and the scalars of the decision — one text line per launch ("tag kernel=... grid=XxYxZ block=N
 * key=value ..."), then the conv and FC forward lines of a one-row f32 forward (the act / evaluate_q shape, tags "act_...").
 * rb_opts: an RB_OPTS string (NULL = all defaults; the environment is NOT read); n_cu: compute units to plan for; flags:
 * RB_LEARNER_* bits; world > 1: the replica exchange is set; with_sink: a priority sink is set.  The lines come from the very
 * plan functions the launchers call (csrc/learner_plan.h).  RB_ERR_INVALID when `cap` bytes are too few.                     */
int rb_debug_launch_plan(const rb_learner_config_t* cfg, const char* rb_opts, int32_t n_cu, int32_t flags, int32_t world,
                         int32_t with_sink, char* out, int64_t cap);

/* The five buffers are caller-owned flat f32 buffers of rb_learner_sizes floats (n_params: both parameter buffers and grads_dev;
 * n_noise: both noise buffers) and must outlive the handle.  grads_dev is ZERO-FILLED by this call: a learn call writes the
 * tensors' elements only, while the gradient norm of the fallback / all-reduce route (one sum of squares over the whole flat
 * buffer) and the optimiser pass sweep the alignment padding between the tensors as well — it must stay zero, so a caller that
 * overwrites grads_dev (an all-reduce, rb_learner_grads_modified) keeps zeros there.  The same padding of the parameter buffers
 * and of the Adam moments is updated with that zero gradient and is never read into a result.                                 */
int rb_learner_create(rb_learner_t** out, const rb_learner_config_t* cfg, float* online_params_dev,
                      float* target_params_dev, float* grads_dev, float* online_noise_dev,
                      float* target_noise_dev, uint64_t seed);
int rb_learner_destroy(rb_learner_t* l);

/* DQN.reset_noise (model.py:82-85, 36-40).  which: 0 online (agent.py:49-50),
 * 1 target (agent.py:74), 2 both in one launch (online first; device RNG only).
 * raw_normals_dev: NULL = device Philox + Box-Muller;
 * else N(0,1) draws in the reference's order (per layer randn(in) then randn(out);
 * layers fc_h_v, fc_h_a, fc_z_v, fc_z_a) — parity hook.                             */
int rb_learner_reset_noise(rb_learner_t* l, int32_t which, const float* raw_normals_dev,
                           rb_stream_t stream);
int64_t rb_learner_noise_draws(const rb_learner_config_t* cfg);
/* The same resample as rb_learner_reset_noise(l, which, NULL, ...) described as a job another
 * launch can host (rb_replay_sample_fused_noise); nothing is launched here.                  */
int rb_learner_noise_job(rb_learner_t* l, int32_t which, rb_noise_job_t* out);

/* Agent.act / evaluate_q (agent.py:53-55, 110-112): single state f32[history][7056]
 * in [0,1]; writes argmax action (i32) and its expected value (f32).
 * noisy=0 is online_net.eval() (mu only, model.py:46).                              */
int rb_learner_act(rb_learner_t* l, const float* state_dev, int32_t noisy, int32_t* action_dev,
                   float* q_dev, rb_stream_t stream);
/* rb_learner_act for a caller that needs the result on the HOST at once (agent.py:53-55 returns a Python int; main.py:153 feeds it to
 * the emulator): action_pinned / q_pinned are PINNED host words mapped on the device (hipHostMalloc / torch pin_memory); the call
 * presets the action word, launches, polls the word in a compiled loop (falling back to a stream synchronise after ~10 ms) and
 * returns the action and its value through action_out / q_out (either may be NULL).  One call instead of launch + a Python poll loop.
 * Where q_pinned == (float*)(action_pinned + 1) and action_pinned is 8-byte aligned, the device writes both with ONE 8-byte store
 * (otherwise: q, a system-scope fence, then the action): rb_learner_act behaves the same way.                                    */
int rb_learner_act_wait(rb_learner_t* l, const float* state_dev, int32_t noisy, int32_t* action_pinned, float* q_pinned,
                        int32_t* action_out, float* q_out, rb_stream_t stream);
/* The same for n states at once (vectorised actors; the reference acts on one state per call,
 * main.py:153 — this is that call batched): states f32[n][history][7056],
 * 1 <= n <= 4096 (beyond the learn step's 3*batch images the forward buffers are regrown once, synchronising — batched
 * evaluation of a validation memory, test.py:38-39); actions_dev i32[n], q_dev f32[n] (either may be NULL).  action_dev /
 * q_dev of both calls may point to pinned host memory mapped on the device, which saves the
 * caller a device-to-host copy: the values are final once the stream has drained.         */
int rb_learner_act_batch(rb_learner_t* l, const float* states_dev, int32_t n, int32_t noisy,
                         int32_t* actions_dev, float* q_dev, rb_stream_t stream);

/* rb_learner_act_batch with Agent.act_e_greedy's draw (agent.py:58-59; test.py:26 evaluates with epsilon = 0.001) inside the
 * head kernel: the same forward, the same n range and buffer growth; only the action selection differs.  For image i of the
 * call, with row = row0 + i:
 *   (x0, x1, ., .) = Philox4x32-10(key = rng_seed, counter = (lo = rng_round, hi = row))     the generator of the device Catch
 *   u = (float)(x0 >> 8) * 2^-24                                                              24 bits, in [0, 1)
 *   explore iff u < epsilon (a float32 compare: epsilon = 0 never explores, epsilon >= 1 always does)
 *   actions_dev[i] = x1 % actions if explored, else the greedy action of rb_learner_act_batch
 *   q_dev[i] (optional) = the GREEDY action's value either way (what evaluate_q returns, agent.py:110-112)
 *   explored_dev[i] (optional, u8) = 1 or 0
 * The generator is counter-based and keeps no state on the device: the same (rng_seed, rng_round, row) gives the same draw
 * again, and because a row's draw depends on row0 + i only, a caller that splits its states over several calls passes the
 * offset of each part as row0 and gets what one call would have given.  n >= 2: the draw lives in the head kernel (no launch
 * of its own); n == 1: the one-launch act path, then one wave that applies the draw to the stored action.
 * Refused with RB_ERR_INVALID and a message: NaN or negative epsilon, NULL actions_dev, row0 < 0.                         */
int rb_learner_act_batch_eps(rb_learner_t* l, const float* states_dev, int32_t n, int32_t noisy, float epsilon,
                             uint64_t rng_seed, uint64_t rng_round, int32_t row0, int32_t* actions_dev, float* q_dev,
                             uint8_t* explored_dev, rb_stream_t stream);

/* One noise sample PER ROW for the batched act path (vectorised actors: stream s explores with its own perturbation of the
 * weights; the reference has one environment and never meets the question).  Fills the caller-owned noise_rows_dev, f32
 * [rows][n_noise]: every row has the layout of rb_learner_noise_layout, n_noise from rb_learner_sizes (its padding included);
 * floats of a row that no tensor of the layout covers are written as zero.  rows in [1, 256], row0 >= 0.
 * raw_normals_dev != NULL (parity hook, as in rb_learner_reset_noise): f32 [rows][rb_learner_noise_draws] of N(0,1) draws in
 * the reference's order; row i is written from its own block.
 * raw_normals_dev == NULL: the device Philox + Box-Muller of rb_learner_reset_noise — the same f(x) = sign(x) sqrt|x|, the same
 * two normals per Philox block — keyed WITHOUT any device state: for row r = row0 + i, draws 2j and 2j + 1 come from
 *   Philox4x32-10(key = rng_seed, counter = (hi = rng_round, lo = ((uint64)r << 32) | j)).
 * The learner's own epoch counter is neither read nor advanced (learner resamples and graph replays are untouched); a row's
 * values depend on (rng_seed, rng_round, r) only, so a caller that splits its rows over several calls passes each part's first
 * row as row0 and gets what one call would have given.
 * Refused with RB_ERR_INVALID and a message naming the argument, before anything is launched: NULL l or noise_rows_dev, rows
 * outside [1, 256], row0 < 0.                                                                                            */
int rb_learner_noise_rows(rb_learner_t* l, int32_t rows, int32_t row0, uint64_t rng_seed, uint64_t rng_round,
                          const float* raw_normals_dev, float* noise_rows_dev, rb_stream_t stream);
/* The forward of rb_learner_act_batch (training mode) with row i's noisy layers under noise row i of noise_rows_dev (f32
 * [n][n_noise], as rb_learner_noise_rows writes it): states f32[n][history][7056], 1 <= n <= 256 (beyond the learn step's
 * 3*batch images the forward buffers are regrown once, synchronising; the first call also allocates two scaled-activation
 * buffers).  actions_dev i32[n], q_dev f32[n]: either may be NULL, both may be pinned host memory.  n == 1 runs the same
 * kernels (not the one-launch act path).  The noisy layers are computed in the factorised form
 *   y[m][j] = sum_k x[m][k] mu[j][k] + eo[m][j] * sum_k (x[m][k] ein[m][k]) sigma[j][k] + bmu[j] + bsigma[j] eo[m][j]
 * so that mu and sigma are streamed ONCE for all rows; this is not the rounding order of the reference (model.py:39,44 forms
 * W = mu + sigma * (eo ein^T) per sample, then contracts) — q agrees with the per-row reference within the act tolerance
 * (rtol 2e-5, atol 1e-6), not to the bit, and an all-zero noise row gives rb_learner_act_batch(noisy = 0) within the same.
 * Refused with RB_ERR_INVALID and a message naming the argument, before anything is launched: NULL l, states_dev or
 * noise_rows_dev, n outside [1, 256].                                                                                    */
int rb_learner_act_batch_rows(rb_learner_t* l, const float* states_dev, int32_t n, const float* noise_rows_dev,
                              int32_t* actions_dev, float* q_dev, rb_stream_t stream);

/* Agent.learn minus sampling/optimiser (agent.py:66-96): three forwards, double-Q
 * select, C51 projection, weighted cross-entropy, full backward into grads_dev.
 * Inputs are rb_replay_sample's outputs.  loss_dev f32[B] = per-sample CE (agent.py:94),
 * i.e. the new raw priorities (agent.py:100).                                        */
int rb_learner_learn(rb_learner_t* l, const uint8_t* states_dev, const uint8_t* next_states_dev,
                     const int64_t* actions_dev, const float* returns_dev,
                     const float* nonterminals_dev, const float* weights_dev, float* loss_dev,
                     rb_stream_t stream);

/* Same step, zero-copy input: instead of gathered stacks the first conv layer reads its frames
 * straight from the replay ring (rb_replay_buffers_t.frames_dev) through the window table the
 * last rb_replay_sample wrote (rb_replay_buffers_t.window_dev: [B][history+multi_step] ring
 * indices, -1 = blanked frame, memory.py:112-121).  Call rb_replay_sample with states_dev =
 * next_states_dev = NULL to skip the gather.                                                 */
int rb_learner_learn_windows(rb_learner_t* l, const uint8_t* frames_dev, const int32_t* windows_dev,
                             int32_t window_len, const int64_t* actions_dev, const float* returns_dev,
                             const float* nonterminals_dev, const float* weights_dev, float* loss_dev,
                             rb_stream_t stream);
/* 1 when rb_learner_learn_windows is available for this handle (the ring-reading first conv
 * layer needs history <= 4 and the LDS conv kernels), else 0: gather and call rb_learner_learn. */
int rb_learner_zero_copy_ok(rb_learner_t* l);

/* clip_grad_norm_ (agent.py:97): global L2 norm of grads_dev, scale in place by
 * max_norm/(norm+1e-6) when that is < 1.  norm_dev (f32[1], may be NULL) gets ||g||. */
int rb_learner_clip_grad(rb_learner_t* l, float max_norm, float* norm_dev, rb_stream_t stream);

/* clip_grad_norm_ + optimiser.step() (agent.py:97-98, optimiser built at agent.py:46) in one pass
 * over the flat buffers: the clip coefficient is applied to the gradient in registers on its way
 * into torch.optim.Adam's update (amsgrad off, weight_decay 0).  exp_avg_dev / exp_avg_sq_dev:
 * caller-owned f32[n_params] moment buffers (zero before step 1); step: 1-based step number for
 * the bias corrections.  grads_dev is rewritten (scaled) only when the norm exceeds max_norm,
 * as clip_grad_norm_ would leave it.  norm_dev (f32[1], may be NULL) gets ||g||.            */
int rb_learner_clip_adam(rb_learner_t* l, float max_norm, float* exp_avg_dev, float* exp_avg_sq_dev,
                         double lr, double beta1, double beta2, double eps, int64_t step,
                         float* norm_dev, rb_stream_t stream);

/* One whole training step of Agent.learn (agent.py:63-100) in ONE call: rb_replay_sample_fused_noise (zero-copy: no stack
 * gather), rb_learner_learn_windows on the frames/windows of `replay`, rb_learner_clip_adam — the same three entry points
 * with the same arguments, back to back.  Why it exists: the HIP runtime lets the launching thread run only about one
 * kernel ahead of the GPU, so host work BETWEEN launches (a Python interpreter between three ctypes calls: ~10 us twice
 * per step) shows up as idle GPU time (measured 2 x 6 us of a 194 us step); inside one call the launches are 3 us apart.
 * The priority write-back needs rb_learner_set_priority_sink(l, replay, tree_idx_dev) set beforehand.               */
typedef struct {
  rb_replay_t* replay;
  int32_t batch, max_attempts, window_len, reserved;
  double priority_weight;
  int64_t* tree_idx_dev;            /* sampler outputs (device, [batch]) */
  int64_t* actions_dev;
  float* returns_dev;
  float* nonterminals_dev;
  float* weights_dev;
  const rb_noise_job_t* noise_job;  /* from rb_learner_noise_job */
  const uint8_t* frames_dev;        /* rb_replay_buffers: frame ring and the sampler's window table */
  const int32_t* windows_dev;
  float* loss_dev;                  /* f32[batch]: per-sample loss (agent.py:94) */
  float* exp_avg_dev;               /* rb_learner_clip_adam arguments */
  float* exp_avg_sq_dev;
  float* norm_dev;
  double lr, beta1, beta2, eps;
  int64_t step;
  float max_norm;
  float reserved2;
} rb_train_step_t;
int rb_learner_train_step(rb_learner_t* l, const rb_train_step_t* a, rb_stream_t stream);

/* Learner options.
 * RB_LEARNER_FUSE_FC_H_DW: the hidden layer's weight gradient (93 % of all gradient bytes) is a rank-B product of two
 *   L2-resident matrices.  With this flag (and batch <= 32) rb_learner_learn* computes it for the global norm only and
 *   does NOT store it; rb_learner_clip_adam then recomputes each 16 x 64 tile on the MFMA units while it streams that
 *   tile's parameters and moments — 2 x 25.7 MB less HBM traffic per step at the canonical shape.  Contract: the next
 *   call on the handle after rb_learner_learn* must be rb_learner_clip_adam (clip_grad / grads_modified refuse), and
 *   grads_dev does not hold the hidden layer's weight gradient afterwards ...
 * RB_LEARNER_WRITE_FUSED_GRADS: ... unless this flag is set as well: the fused pass then also stores the tiles it
 *   computed (as clip_grad_norm_ leaves them), which is how the parity tests read the product path's gradient.
 * RB_LEARNER_DEFER_UPDATE: rb_learner_train_step (called with step = 0: a device step counter is required) leaves its
 *   clip + Adam pass (agent.py:97-98) PENDING instead of launching it.  The next rb_learner_train_step hosts it as extra
 *   workgroups of its sampler launch: the optimiser pass of learn call k does not depend on the sampling of call k + 1 nor
 *   the other way round (the priorities were written back in call k's backward), so 30 us of pure HBM streaming run
 *   beside the sampler's one latency-bound workgroup instead of in front of it.  Same arithmetic in the same order: the
 *   parameters are bit-identical to the undeferred ones.  EVERY other learner entry point that touches parameters,
 *   moments, gradients or the norm (act, act_batch, learn*, clip_*, sync_target, set_target_tau, target_ema, shrink_perturb, finish_grads, debug_read) first runs the
 *   pending pass as a launch of its own, on the stream it is given — use ONE stream per handle.  A caller that reads the
 *   borrowed buffers itself (params_dev, exp_avg, exp_avg_sq, grads_dev, norm_dev) calls rb_learner_flush first.       */
#define RB_LEARNER_FUSE_FC_H_DW 1
#define RB_LEARNER_WRITE_FUSED_GRADS 2
#define RB_LEARNER_DEFER_UPDATE 4
/* RB_LEARNER_IMPLICIT_SIGMA (with RB_LEARNER_DEFER_UPDATE, batch <= 32): the hidden layer's sigma-weight gradient is
 *   g_mu * (eps_out x eps_in) element for element (the product rule of model.py:44, what the backward forms), so the backward
 *   does not store it and the HOSTED optimiser pass forms it again from g_mu and a snapshot of the noise while it updates the
 *   (mu, sigma) pairs together: 12.85 MB less written and 12.85 MB less read per step at the canonical shape, bit-identical
 *   parameters.  grads_dev lacks that range until rb_learner_flush (which materialises it), rb_learner_clip_grad or a pass
 *   that runs as a launch of its own; rb_learner_grads_modified refuses while it is missing.                          */
#define RB_LEARNER_IMPLICIT_SIGMA 8
int rb_learner_set_flags(rb_learner_t* l, int32_t flags);
/* Run the pending optimiser pass, if any (RB_LEARNER_DEFER_UPDATE), on `stream`.  No-op otherwise.                    */
int rb_learner_flush(rb_learner_t* l, rb_stream_t stream);
/* The same deferral for a caller that issues a step's entry points one by one (rainbow_amd.Agent's eager path; the replica
 * exchange of SURVEY 8(e), where finish_grads sits between the backward and the optimiser pass, agent.py:96-97):
 *   rb_learner_clip_adam_deferred = rb_learner_clip_adam, but the pass is left pending when the flag is set and it can be
 *     (step = 0 with a device step counter; otherwise it runs at once);
 *   rb_learner_attach_pending(l, job_in, batch, job_out): job_out = job_in (from rb_learner_noise_job) plus the pending pass;
 *     returns 1 if one was attached, 0 if job_out is a plain copy, < 0 on error.  Pass job_out to
 *     rb_replay_sample_fused_noise, then call rb_learner_pending_launched(l).  No other call on the handle in between.  */
int rb_learner_clip_adam_deferred(rb_learner_t* l, float max_norm, float* exp_avg_dev, float* exp_avg_sq_dev, double lr,
                                  double beta1, double beta2, double eps, int64_t step, float* norm_dev, rb_stream_t stream);
int rb_learner_attach_pending(rb_learner_t* l, const rb_noise_job_t* job_in, int32_t batch, rb_noise_job_t* job_out);
int rb_learner_pending_launched(rb_learner_t* l);

/* hipGraph replay with the fused optimiser pass: a captured launch cannot take a new `step` by value.  With a counter set
 * (caller-owned i64 on the device), every rb_learner_learn* increments it on the device, and rb_learner_clip_adam called
 * with step = 0 reads the step number from it and forms the bias corrections 1 - beta^t in the kernel (double, one thread
 * per block).  NULL clears.                                                                                           */
int rb_learner_set_step_counter(rb_learner_t* l, int64_t* step_dev);

/* The learner's side of rb_replay_set_horizon: 1 <= n_eff <= cfg.multi_step, 0 < discount <= 1.  Sets the head's
 * gamma_n = float32(pow(discount, n_eff)) (agent.py:79) and the next-state slot n_eff + c that the zero-copy conv path reads from a
 * window-table row; the row stride that rb_learner_learn_windows checks stays history + cfg.multi_step.  Host state read when a step
 * is launched: no launch, no stream.  rb_learner_train_step* draw the batch themselves and refuse, before anything is launched, when
 * the replay's (n_eff, discount) differ from the learner's; a caller that samples itself (rb_learner_learn, rb_learner_learn_windows)
 * keeps the two handles in step.                                                                                          */
int rb_learner_set_horizon(rb_learner_t* l, int32_t n_eff, double discount);
int rb_learner_get_horizon(rb_learner_t* l, int32_t* n_eff_host, double* discount_host);

/* Fused priority write-back (agent.py:100 -> memory.py:157-159).  With a sink set, rb_learner_learn*
 * itself applies  sum_tree[tree_idx] = loss^w  (+ ancestor sums, max) to `replay` as one extra
 * workgroup of its backward launch, i.e. off the step's critical path.  tree_idx_dev must be the
 * index buffer the sampler fills each step (i64[batch]).  rb_learner_priority_written() tells
 * whether the LAST learn call did the write-back (it does not on the generic fallback path or
 * for batch > 256; the caller then calls rb_replay_update_priorities as usual).  Pass NULLs to
 * clear the sink.                                                                           */
int rb_learner_set_priority_sink(rb_learner_t* l, rb_replay_t* replay, const int64_t* tree_idx_dev);
int rb_learner_priority_written(rb_learner_t* l);

/* ---- Replica exchange (the reference is single-device, the insert point is between agent.py:96 and :97).
 * Every replica must apply the MEAN gradient.  27 MB of it are the noisy-linear weight gradients, and those are rank-B
 * products  dW = dY^T X  of two thin matrices: instead of all-reducing dW (2 x 7/8 x 27 MB through each GPU's xGMI links),
 * the replicas all-gather the FACTORS (dlogits, h, dh, feat rows of their batch, their noise vectors) and each computes the
 * mean gradient of the global batch from the gathered rows itself — identical inputs, identical kernel, identical bits on
 * every replica.  The conv gradients (the leading `small_floats` of grads_dev, 0.3 MB) ride in the SAME block, so a step
 * needs exactly ONE collective (an all-gather of `factor_floats` = 1.0 MB per rank at the canonical shape) and no event or
 * side stream (round 2 all-gathered the FC factors on a side stream under the backward and all-reduced the conv range
 * separately: two collectives, two stream joins — 75 us of idle GPU per step in the one-rank plumbing run).
 *   rb_learner_set_exchange(world > 1, local block, gathered blocks [world][factor_floats])   once
 *   per step:  rb_learner_learn*            input-gradient chain, conv grads, the complete local block; NO FC weight grads
 *              [caller: all-gather the local blocks into the gathered buffer, on the learn call's stream]
 *              rb_learner_finish_grads      FC weight/bias gradients of the global batch and the conv gradients' replica
 *                                           mean (rank order, x 1/world) into grads_dev + the norm partials
 *              rb_learner_clip_adam / rb_learner_clip_grad as usual
 * rb_learner_wait_factors is kept for ABI compatibility and does nothing (the block is complete in stream order).
 * world == 1 (default) restores the single-device step.  [small_offset, +small_floats) still names the conv range for
 * hosts that prefer `allreduce` of the flat gradient + rb_learner_grads_modified.
 * One rank's block is six segments, each rounded up to 64 floats:
 *   dlogits [B][NZ] | h [B][2H] | dh [B][2H] | feat [B][F] | noise [n_noise] | conv grads [small_floats]
 * (factor_floats is their total).  The learn call writes the tensors' elements only: the gaps between the segments are never
 * read, but the alignment padding BETWEEN the conv tensors lies inside the conv segment and is folded (and squared into the
 * norm) with it — allocate the local block zero-filled, as grads_dev is.
 * rb_learner_set_exchange refuses with RB_ERR_STATE and a message that points to the `allreduce` route: world outside [1, 64]
 * (RB_ERR_INVALID), a shape off the streamed noisy-linear kernels (hidden % 32 != 0, hidden > 4096), and a shape whose
 * rb_learner_finish_grads launch would need more sum-of-squares slots than the 16 384 that exist (8 per 128 x 128 tile of the
 * hidden layer's weights and per 16-row x 512-column tile of the output layer's, one per hidden-layer tile for the conv range:
 * canonical, hidden 4096, 18 actions needs 18 368).                                                                     */
int rb_learner_exchange_layout(rb_learner_t* l, int64_t* factor_floats, int64_t* small_offset, int64_t* small_floats);
int rb_learner_set_exchange(rb_learner_t* l, int32_t world, float* factors_local_dev, const float* factors_all_dev);
int rb_learner_wait_factors(rb_learner_t* l, rb_stream_t side_stream);
int rb_learner_finish_grads(rb_learner_t* l, rb_stream_t stream);

/* The same exchange WITHOUT a host framework in the loop: the library issues the all-gather itself on an RCCL
 * communicator it owns (librccl is resolved at run time with dlopen — the library has no link-time dependency on it), so a
 * C / C++ host needs no torch.distributed, and the Python host saves the ~16 us per step torch.distributed spends around a
 * 1 MB collective (profiles/round3_defer_dist1.txt).  One communicator per process / GPU:
 *   rank 0:     rb_comm_unique_id(id)                  128 opaque bytes (ncclGetUniqueId); ship them to every rank out of band
 *   every rank: rb_comm_create(&comm, id, world, rank) ncclCommInitRank on the CURRENT device (collective: all ranks call it)
 *   per step:   rb_learner_exchange_rccl(l, comm, stream)  =  ncclAllGather(local block -> gathered blocks) on `stream`
 *                                                             + rb_learner_finish_grads(l, stream)
 * A one-rank communicator with a two-block exchange buffer (the single-GPU plumbing run, RAINBOW_AMD_FORCE_DIST=1) gathers
 * into block 0 and copies it to block 1.  Replaces the [caller: all-gather] step above; insert point agent.py:96-97.        */
typedef struct rb_comm rb_comm_t;
/* 1 when librccl can be loaded by this process (dlopen + symbol lookup only: creates nothing), else 0.  What every rank asks
 * before the group decides whether to build library-owned communicators; only rank 0 then calls rb_comm_unique_id.          */
int rb_comm_available(void);
int rb_comm_unique_id(void* id128);
int rb_comm_create(rb_comm_t** out, const void* id128, int32_t world, int32_t rank);
int rb_comm_destroy(rb_comm_t* comm);   /* waits for the stream of the communicator's last all-gather first */
int rb_learner_exchange_rccl(rb_learner_t* l, rb_comm_t* comm, rb_stream_t stream);
/* rb_learner_train_step with the exchange in its place (sampler + noise, learn, exchange_rccl, clip + Adam): the replica
 * step as ONE C call.  Needs rb_learner_set_exchange to be armed for comm's world size.                                  */
int rb_learner_train_step_dist(rb_learner_t* l, const rb_train_step_t* a, rb_comm_t* comm, rb_stream_t stream);

/* Tell the library the caller changed grads_dev after rb_learner_learn (e.g. the RCCL
 * all-reduce of the replica path): the sum of squares the backward kernels accumulated on
 * the fly is then stale and rb_learner_clip_grad re-reads the gradient.                    */
int rb_learner_grads_modified(rb_learner_t* l);

/* Exact resume: the noise generator is Philox(seed, epoch, index) with a device-resident epoch that
 * every resample advances; a checkpoint that carries (seed, epoch) — next to parameters, Adam moments and the noise
 * buffers — continues the very same random stream.  Both calls synchronise `stream`.                               */
int rb_learner_get_rng(rb_learner_t* l, uint64_t* seed_host, uint64_t* epoch_host, rb_stream_t stream);
int rb_learner_set_rng(rb_learner_t* l, uint64_t seed, uint64_t epoch, rb_stream_t stream);

/* Agent.update_target_net (agent.py:102-103): params AND noise, device-to-device.   */
int rb_learner_sync_target(rb_learner_t* l, rb_stream_t stream);

/* A target network that follows EVERY optimiser step (DrQ / SPR: tau = 1; SR-SPR / BBF: tau = 0.005) instead of being copied
 * every few thousand: target <- target + tau * (online - target), element for element on the PARAMETERS (the target's noise is
 * redrawn before every use and is left alone; rb_learner_sync_target keeps working and keeps copying both).
 * rb_learner_set_target_tau: tau in [0, 1] (anything else: RB_ERR_INVALID).  A pending optimiser pass runs first, with the tau
 *   it was issued under.  From then on every optimiser pass the library issues (rb_learner_clip_adam, _deferred,
 *   rb_learner_train_step[_dist]) moves the target INSIDE the pass, right behind the parameter update, where the new value is
 *   still in a register: no launch of its own, the pass stays hosted by the next sampler launch (RB_LEARNER_DEFER_UPDATE), and
 *   the only extra traffic is the target array itself — read and written for tau < 1, only written for tau = 1 (the target
 *   then equals the online parameters bit for bit).  Under RB_LEARNER_FUSE_FC_H_DW the EMA is one small launch behind the
 *   pass instead.  A step the pass skips (failed draw) does not move the target either.  tau = 0 (the default) switches it off:
 *   every launch is then exactly what it is without this call.  With a pass pending the target is one step behind, like the
 *   parameters: rb_learner_flush before reading target_params_dev.
 * rb_learner_target_ema: ONE such step now, unconditionally, as a launch of its own (a pending pass runs first): for a caller
 *   whose optimiser is not the library's (call it right after that optimiser's step).  tau = 0 does nothing.              */
int rb_learner_set_target_tau(rb_learner_t* l, float tau, rb_stream_t stream);
int rb_learner_target_ema(rb_learner_t* l, float tau, rb_stream_t stream);

/* Shrink-and-perturb reset (the periodic resets of SR-SPR / BBF, which make a replay ratio above 1 work): per named tensor of
 * rb_learner_param_layout   theta <- alpha * theta + (1 - alpha) * phi,   phi a FRESH draw from the tensor's initial distribution
 * (convs.*: U(+-1/sqrt(fan_in)); *_mu: U(+-1/sqrt(in)); weight_sigma = noisy_std/sqrt(in) and bias_sigma = noisy_std/sqrt(out)
 * are constants: phi is that constant).  convs.* take alpha_encoder, fc_* take alpha_head; both in [0, 1], anything else (NaN
 * too) is RB_ERR_INVALID.  ONE launch over the flat buffers, in stream order, no synchronisation, no host draw.
 *   A pending optimiser pass runs FIRST (it was computed for the old tensors).
 *   phi of flat element i is word i & 3 of Philox4x32-10(key = seed ^ 0x5245534554, counter hi = draw, lo = i >> 2):
 *     u = (float)(x >> 8) * 2^-24, phi = bound * (2u - 1), bound rounded to f32; new = alpha * theta + (1.0f - alpha) * phi as two
 *     products and a sum.  It depends on (seed, draw, i) only: replicas that pass the same pair draw the same phi, and a resumed
 *     run repeats it bit for bit.  The caller advances `draw` once per reset.
 *   alpha == 1: the tensor and its moments are neither read nor written.  alpha == 0: phi is written without reading theta.
 *   with_target != 0: the target parameters get the same rule with the SAME phi (alpha == 0: online and target bit-equal).
 *   exp_avg_dev / exp_avg_sq_dev [n_params] (both or neither; NULL = no moments to clear): zeroed for every tensor with alpha < 1.
 *   The alignment padding between the tensors is never written; gradients, noise, the step counter and the replay are untouched. */
int rb_learner_shrink_perturb(rb_learner_t* l, float alpha_encoder, float alpha_head, float noisy_std, uint64_t seed, uint64_t draw,
                              int32_t with_target, float* exp_avg_dev, float* exp_avg_sq_dev, rb_stream_t stream);

/* ---- device-side diagnostics (all off by default: with none of them used, every launch, grid and result is what it is
 * without this section).
 *
 * Step records.  One 64-byte record per learn call, written by the device into a ring the caller owns and read whenever the
 * caller likes: watching a loss curve no longer means reading a private buffer behind a synchronise after every step.   */
typedef struct {
  int64_t step;        /* the device step counter as this call's head kernel left it; -1 without one (rb_learner_set_step_counter) */
  int32_t batch;       /* B */
  int32_t status;      /* the call's batch status word (non-zero: the sampler gave up, the weights are zero); 0 without a sink */
  float loss_mean, loss_max;      /* over loss_dev[b] (agent.py:94) */
  float wloss_mean;               /* mean_b w_b * loss_b: the objective of agent.py:96 */
  float weight_mean;              /* mean_b w_b */
  float q_mean;                   /* mean_b sum_z support[z] * exp(log p(s_t, a_t)[b][z]): the online value of the taken action */
  float q_target_mean;            /* mean_b sum_z support[z] * m[b][z]: the projected target's value */
  float td_abs_mean;              /* mean_b |q_target_b - q_b| */
  float entropy_mean;             /* mean_b -sum_z p log p of p(s_t, a_t) */
  float return_mean;              /* mean_b returns[b] */
  float terminal_frac;            /* share of rows with nonterminals[b] == 0 */
  float grad_norm;                /* the gradient's global norm BEFORE the clip; NaN when the call left no partial list (below) */
  float reserved;                 /* written as 0 */
} rb_step_stats_t;                /* 64 bytes */

/* ring_dev [capacity] records and count_dev (one device word, zeroed by the caller) are caller-owned; NULL / NULL (capacity is then
 * ignored) switches the records off again.  With a ring set, every learn call — rb_learner_learn, rb_learner_learn_windows,
 * rb_learner_train_step[_dist] — ends with ONE extra launch behind its last backward kernel, which writes the record at
 * *count_dev % capacity and then increments *count_dev: both on the device, so a captured graph replays them correctly.  All 64
 * bytes are written every time (the ring may be a never-zeroed allocation), nothing outside the ring and the word is.  The record
 * is a fixed-order reduction (double accumulation, rows in index order): bit-identical from run to run.
 *   grad_norm is summed from the partial sums of squares the backward kernels left, in the optimiser pass's own order, so it
 *     equals bit for bit what that pass later stores to norm_dev; the list is read, not consumed.  It is NaN when the call left
 *     none: the fallback kernels (RB_OPTS generic), and the replica exchange, where the gradient is complete only after
 *     rb_learner_finish_grads.  It is always the norm of the gradient THIS call computed: a caller that changes grads_dev afterwards
 *     and says so with rb_learner_grads_modified (an all-reduce over replicas) gets the norm of the changed gradient in norm_dev,
 *     and the record keeps the local one: then neither NaN nor equal to norm_dev.
 *   A failed draw gives a record with status != 0 and an unchanged step.
 * The first call with a ring allocates a few KB of scratch in the handle, which synchronises the device once: make it before
 * capturing a graph.  Reading: synchronise the stream the learn calls went to, copy *count_dev and the ring (rb_copy_to_host);
 * record i of the run sits in slot i % capacity, and the records below *count_dev - capacity are overwritten.                  */
int rb_learner_set_stats(rb_learner_t* l, rb_step_stats_t* ring_dev, int32_t capacity, int64_t* count_dev);

/* Held-out loss: the learn step's three forwards and its head on a batch the caller supplies, and nothing else — no backward, no
 * priority write-back, no noise draw, no optimiser pass.  Both networks run in eval mode (noise zero, model.py:46), so the result
 * is deterministic; the targets use the handle's horizon (rb_learner_set_horizon) and unit importance weights.
 *   loss_dev [B]: the per-sample cross-entropy.  stats_out_dev (may be NULL): ONE record of the batch, with step = -1, status = 0
 *   and grad_norm = NaN; the ring of rb_learner_set_stats and its count are not touched.
 * State rules of rb_learner_act_batch: a pending optimiser pass runs first.  It overwrites the activations of the last learn call,
 * so it refuses (RB_ERR_STATE) while that call's gradients still wait for rb_learner_finish_grads or for the fused optimiser pass
 * (RB_LEARNER_FUSE_FC_H_DW).  Parameters, target, moments, gradients and their norm partials, both noise buffers and the noise
 * epoch, the step counter and the priority sink's tree are left unchanged, bit for bit.  The first call allocates scratch in the
 * handle and synchronises once.                                                                                           */
int rb_learner_eval_loss(rb_learner_t* l, const uint8_t* states_dev, const uint8_t* next_states_dev,
                         const int64_t* actions_dev, const float* returns_dev, const float* nonterminals_dev,
                         float* loss_dev, rb_step_stats_t* stats_out_dev, rb_stream_t stream);

/* Priority statistics of a replay: one streamed pass over the `capacity` leaves of the sum tree (4 MB at 2^20 slots), in stream
 * order.  A leaf that is NaN, infinite or negative counts as invalid and is excluded from everything else; zero leaves (empty
 * slots, slots kept unsampleable) are counted nowhere.  Leaves are split over workgroups in fixed chunks, every workgroup leaves
 * double partials, and the last one to arrive adds them in chunk order: the result is bit-identical when repeated.            */
typedef struct {
  int64_t nonzero, invalid;    /* leaves > 0 and finite; leaves that are NaN, inf or negative */
  double sum, sumsq;           /* over the valid non-zero leaves (effective sample size = sum^2 / sumsq) */
  float max, min_pos;          /* largest and smallest valid non-zero leaf; 0 and 0 for an empty tree */
  int32_t hist[64];            /* bin k: valid non-zero leaves with floor(log2 p) == k - 40, clamped at both ends; the exponent is
                                  read from the bit pattern, denormals go to bin 0 */
} rb_priority_stats_t;
/* out_dev is overwritten entirely.  Like every reader of the tree it waits for and discards an early draw in flight.  The partial
 * scratch belongs to the handle: it is allocated by the first call, which synchronises the device once.                       */
int rb_replay_priority_stats(rb_replay_t* r, rb_priority_stats_t* out_dev, rb_stream_t stream);

/* ---- dormant units (ReDo: Sokar, Agarwal, Castro, Evci, "The Dormant Neuron Phenomenon in Deep RL", ICML 2023): a targeted reset
 * and the diagnostic that goes with it.  Never on the per-step path: a run that does not call these launches what it launched before.
 *
 * A UNIT is an output channel of a conv layer or a hidden unit of fc_h_v / fc_h_a.  The layers, in this order: conv 0 .. nconv - 1
 * (cout units each), fc_h_v (hidden units), fc_h_a (hidden units); U = the sum, the units numbered in that order.
 * rb_learner_unit_layout: *n_layers = nconv + 2 and units_per_layer[5] (may be NULL; entries beyond n_layers are 0).
 *   Incoming parameters of unit i: conv layer l: row i of convs.l.weight and convs.l.bias[i]; hidden unit j of stream s: row
 *   s * hidden + j of fc_h weight_mu and weight_sigma, and its bias_mu and bias_sigma.
 *   Outgoing parameters: conv l < nconv - 1: the ks^2 floats at o * K' + i * ks^2 of every row o of the next conv weight; the last
 *   conv layer: columns [i P, (i + 1) P) of all 2 * hidden rows of fc_h weight_mu and weight_sigma; hidden unit j of stream v / a:
 *   column j of fc_z_v's / fc_z_a's weight_mu and weight_sigma.                                                                */
int rb_learner_unit_layout(const rb_learner_config_t* cfg, int32_t* n_layers, int32_t* units_per_layer);

/* The ONLINE network's forward in eval mode (noise zero, as rb_learner_eval_loss) on B = cfg.batch states u8 [B][history][84][84] —
 * no target rows, no head — then ONE launch that writes (accumulate == 0) or adds to (!= 0)
 *   activity_dev[i] = sum over the B rows and the unit's positions of its post-ReLU activation          double [U]
 * accumulated in double in a fixed order: a repeated call is bit-identical.  State rules of rb_learner_eval_loss: a pending
 * optimiser pass runs first; RB_ERR_STATE while the last learn call's gradients wait for rb_learner_finish_grads or for the fused
 * optimiser pass (the call overwrites that call's activations); parameters, target, moments, gradients and their norm partials,
 * both noise buffers and the noise epoch, the step counter and the priority sink's tree are unchanged, bit for bit.             */
int rb_learner_unit_activity(rb_learner_t* l, const uint8_t* states_dev, int32_t accumulate, double* activity_dev, rb_stream_t stream);

/* ONE launch.  S_l = the fixed-order double sum of layer l's N_l activities; unit i is dormant iff activity[i] * N_l <= tau * S_l in
 * double — the paper's s_i = E|h_i| / mean_k E|h_k| <= tau without the division (the sample count cancels inside a layer).  An
 * all-zero layer is dormant as a whole.  A NaN makes the comparison false: a unit whose activity is NaN is never recycled, and a NaN
 * in a layer (S_l is then NaN) recycles nothing in that layer.
 *   mask_dev u8 [U]: 1 = dormant.  counts_dev i32 [n_layers]: dormant units per layer.  scores_dev float [U] (may be NULL):
 *   (float)(activity[i] * N_l / S_l), 0 where S_l == 0.  tau must be finite and >= 0 (NaN too is RB_ERR_INVALID).                */
int rb_learner_dormant_mask(rb_learner_t* l, const double* activity_dev, double tau, uint8_t* mask_dev, int32_t* counts_dev,
                            float* scores_dev, rb_stream_t stream);

/* The targeted reset.  A pending optimiser pass runs FIRST; then ONE launch in stream order: the mask is never read by the host and
 * nothing synchronises.  For every unit with mask_dev[i] != 0:
 *   incoming parameters <- phi, a fresh draw from the tensor's initial distribution (the bounds and constants of
 *     rb_learner_shrink_perturb).  phi of flat element e is word e & 3 of Philox4x32-10(key = seed ^ 0x5245444F, counter hi = draw,
 *     lo = e >> 2): u = (float)(x >> 8) * 2^-24, phi = bound * (2u - 1); the sigma tensors take their constant.  phi is written
 *     without reading theta (a NaN does not survive) and depends on (seed, draw, e) alone: not on which other units are dormant.
 *   outgoing parameters: weight_mu and conv weights <- 0, weight_sigma <- its initial constant, so that the eval-mode function of
 *     the network is unchanged and the unit starts like a fresh noisy connection.  An element that is incoming to one dormant unit
 *     and outgoing from another gets the outgoing rule (zero wins).
 *   exp_avg_dev / exp_avg_sq_dev [n_params] (both or neither; NULL = none): zeroed at every written element.
 *   with_target != 0: the target parameters get the same values, the same phi.
 * Everything else is neither read nor written: the elements of units that are not dormant, the alignment padding, the output layer's
 * biases, gradients, noise, the step counter.  With no dormant unit no byte changes.                                            */
int rb_learner_recycle_units(rb_learner_t* l, const uint8_t* mask_dev, float noisy_std, uint64_t seed, uint64_t draw,
                             int32_t with_target, float* exp_avg_dev, float* exp_avg_sq_dev, rb_stream_t stream);

/* ---- feature rank (srank: Kumar, Agarwal, Ghosh, Levine, ICLR 2021; feature rank: Lyle, Rowland, Dabney, ICLR 2022) and per-tensor
 * norms: the two loss-of-plasticity diagnostics beside the dormant-unit share.  Never on the per-step path: a run that does not call
 * these launches what it launched before.
 *
 * The features of a state: RB_FEATURES_HIDDEN, the post-ReLU row [fc_h_v | fc_h_a], d = 2 * hidden; RB_FEATURES_CONV, the last conv
 * layer's post-ReLU output flattened, d = F (what fc_h reads).  rb_learner_feature_dim: *d of a configuration; no device needed. */
#define RB_FEATURES_HIDDEN 0
#define RB_FEATURES_CONV 1
int rb_learner_feature_dim(const rb_learner_config_t* cfg, int32_t which, int32_t* d);

/* The ONLINE network's forward in eval mode on B = cfg.batch states u8 [B][history][84][84] — the forward of
 * rb_learner_unit_activity: noise zero, no target rows, no head — then a copy in stream order, nothing synchronises:
 *   out_dev[b * ld + k] = feature k of row b,   k < d, b < B      float, ld >= d floats between rows
 * Columns [d, ld) of every row are not written.  The rows are bit-equal to what rb_learner_debug_read hands out after the same
 * forward (selector 5; selector 6 + nconv - 1).  State rules of rb_learner_unit_activity: a pending optimiser pass runs first;
 * RB_ERR_STATE while the last learn call's gradients wait for rb_learner_finish_grads or for the fused optimiser pass (the call
 * overwrites that call's activations); parameters, target, moments, gradients and their norm partials, both noise buffers and the
 * noise epoch, the step counter and the priority sink's tree are unchanged, bit for bit.                                        */
int rb_learner_features(rb_learner_t* l, const uint8_t* states_dev, int32_t which, float* out_dev, int32_t ld, rb_stream_t stream);

/* The sample-side Gram matrix of n feature rows, ONE launch, no handle:
 *   gram_dev[i * n + j] = sum_k phi[i * ld + k] * phi[j * ld + k],  k < d        double [n][n], every element written
 * phi_dev: float, n rows of ld floats (all n * ld are addressable).  The inputs are widened exactly and the sum is accumulated in
 * double by v_mfma_f64_16x16x4_f64 (an f32 accumulation leaves a noise floor of sigma_max sqrt(d 2^-24) under the singular values;
 * here it is sigma_max sqrt(d 2^-53)).  One workgroup per 64 x 64 tile pair of the upper triangle; an off-diagonal value is computed
 * once and stored at [i][j] and [j][i]: K is symmetric bit for bit.  The reduction over k is never split: every element is one
 * chain in ascending k, four per MFMA, so the result depends on d alone — not on n, on the grid or on ld; a repeated call is
 * bit-identical and the K of the first m rows is the top-left block of the K of all of them.  Columns [d, ld) and whatever lies
 * behind row n - 1 never enter a sum (they may hold NaN).  |K - K_exact| <= d 2^-53 sum_k |phi_ik| |phi_jk|.
 * RB_ERR_INVALID naming the argument, nothing launched: n outside [1, 4096], d < 1, ld < d, ld % 4 != 0, phi_dev not 16-byte or
 * gram_dev not 8-byte aligned, 4 * n * ld >= 2^31.                                                                               */
int rb_gram_f64(const float* phi_dev, int32_t n, int32_t d, int32_t ld, double* gram_dev, rb_stream_t stream);

/* Per tensor of rb_learner_param_layout, in its order (n_tensors = 2 * nconv + 16), over flat buffers shaped like the parameters
 * (the parameters, the target, the gradient, a moment buffer; 16-byte aligned):
 *   out_dev[3 * t + 0] = sum a^2    out_dev[3 * t + 1] = sum (a - b)^2  (0 when b_dev is NULL)    out_dev[3 * t + 2] = max |a|
 * double [n_tensors][3], accumulated in double in a fixed order (a repeated call is bit-identical); a NaN anywhere in a tensor (a or
 * b) makes all three of ITS values NaN and touches no other tensor; the alignment padding between tensors is never read.  A pending
 * optimiser pass runs first; with a_dev or b_dev = grads_dev an implicit sigma gradient is materialised first, and the call is
 * RB_ERR_STATE while the hidden layer's weight gradient is left to the fused optimiser pass.  TWO launches in stream order (partials
 * of fixed 4096-element chunks; one workgroup per tensor folds them in index order); nothing synchronises, except that a handle's
 * first call allocates the partials' scratch.                                                                                   */
int rb_learner_tensor_norms(rb_learner_t* l, const float* a_dev, const float* b_dev, double* out_dev, rb_stream_t stream);

/* White-box access for parity tests: copies an internal activation to out_dev.
 * what: 0 log_ps_a [B][atoms], 1 m (projected target) [B][atoms], 2 argmax a* i32[B],
 *       3 pns_a [B][atoms], 4 logits [3B][atoms*(actions+1)],
 *       5 hidden activations relu(fc_h_v | fc_h_a) of the differentiated forward [B][2*hidden] (model.py:72-73) — read WITHOUT
 *         running a pending optimiser pass (it is no parameter): h > 0 are the ReLU decisions the backward used;
 *       6, 7, 8 the activations of conv layer 0, 1, 2 of that forward [B][cout][oh][ow], likewise: the ReLU decisions the conv
 *         backward used (RB_ERR_INVALID beyond the network's last conv layer).                                          */
int rb_learner_debug_read(rb_learner_t* l, int32_t what, void* out_dev, rb_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RAINBOW_HIP_H_ */
