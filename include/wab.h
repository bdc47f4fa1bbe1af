/*
 * wab.h — C-ABI of the MI355X-native batched Wolves-and-Bushes step.
 *
 * This is the drop-in boundary for the hot path of johnmatthewtennant/wab-gym:
 * `WolvesAndBushesEnv.reset()/step()` (wab_env.py:103-342) with a leading batch
 * dimension.  Plain pointers and sizes only; every device pointer is a HIP device
 * address (e.g. a torch tensor's data_ptr()), every `stream` a hipStream_t (NULL =
 * the legacy default stream).  The caller owns all I/O buffers; the handle owns
 * per-env state in HBM and the constant tables.  Calls are stream-ordered and
 * asynchronous unless stated otherwise.  A handle is not thread-safe.  All calls
 * return 0 on success and a negative WAB_E_* code on failure; the message is
 * available from wab_last_error() (thread-local).
 *
 * Reference interface replaced (file:line in /root/reference):
 *   wab_config            <- default_game_options                   wab_env.py:11-39
 *   wab_create            <- WolvesAndBushesEnv.__init__            wab_env.py:106-186
 *                            (odd width/height check                wab_env.py:147-148)
 *   wab_reset             <- WolvesAndBushesEnv.reset               wab_env.py:231-248
 *   wab_step              <- WolvesAndBushesEnv.step                wab_env.py:250-342
 *   wab_obs               <- _get_obs 7-tuple                        wab_env.py:359-385
 *   wab_rollout           <- the per-step loop of actor_critic.main  actor_critic.py:185-200
 *                            with pre-chosen actions (T steps)
 *   wab_destroy           <- (gym.Env.close; nothing to free in the reference)
 *   wab_featurize         <- PragmaticObsWrapper.observation         wab_env.py:726-824
 *   wab_featurize_superbasic <- SuperBasicObservationWrapper.observation wab_env.py:900-927
 *   wab_step_features        <- PragmaticObsWrapper(env).step, actor_critic.py:180-192
 *   wab_rollout_features     <- T steps of actor_critic.main's loop     actor_critic.py:185-200
 *                               + finish_episode's returns              actor_critic.py:139-143
 *   wab_render            <- WolvesAndBushesEnv.render (rgb_array,   wab_env.py:468-502
 *                            draw_health text included)
 *   wab_render_envs       <- the same for a range of envs (Monitor video frames)
 *   wab_egocentric        <- WolvesAndBushesEnvEgoCentric._get_obs /  wab_env.py:930-979
 *                            _get_bush_proximities                   wab_env.py:652-667
 *                            + gym.spaces.flatten                    actor_critic.py:188
 *   wab_discounted_returns<- finish_episode's return loop             actor_critic.py:139-143
 *   wab_discounted_returns_exact <- the same on the env's own rewards   actor_critic.py:139-145
 *   wab_episode_stats_update <- gym.wrappers.Monitor's episode returns   actor_critic.py:46,
 *                            and lengths, over a [T][B] segment          210-224
 *   wab_normalize_episode_returns <- finish_episode's (R - mean) /       actor_critic.py:145-146
 *                            (std + eps), per episode
 *   wab_gae               <- (no counterpart: the reference plays whole episodes and uses
 *                            R - value, actor_critic.py:149; a fixed [T][B] segment needs the
 *                            bootstrapped, lambda-weighted form)
 *   wab_whiten            <- finish_episode's (x - mean) / (std + eps)  actor_critic.py:145-146
 *                            over a whole tensor instead of one episode
 *   wab_snapshot_save / wab_snapshot_restore <- (no counterpart: the reference has no
 *                            checkpoint, resume or rewind of an env)
 *   wab_policy_act        <- Policy.forward + select_action's sample  actor_critic.py:76-125
 *   wab_rollout_policy    <- T steps of actor_critic.main's loop with   actor_critic.py:108-125,
 *                            select_action choosing each action          185-200
 *   wab_policy_grad       <- finish_episode's loss and loss.backward()  actor_critic.py:148-165
 *   wab_policy_grad_ppo   <- the same with PPO's clipped surrogate; wab_policy_evaluate its old_logp
 *   wab_policy_adam_step  <- optimizer.step() (optim.Adam)              actor_critic.py:104, 165
 */
#ifndef WAB_H_
#define WAB_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WAB_ABI_VERSION 14
#define WAB_MAX_WOLF_SLOTS 32 /* largest per-env live-wolf slot count (wab_config.wolf_slots) */
#define WAB_MAX_VIEW 63       /* largest odd width/height accepted */

/* error codes */
#define WAB_OK 0
#define WAB_E_INVALID (-1)    /* bad argument (ValueError in the reference) */
#define WAB_E_HIP (-2)        /* HIP runtime error */
#define WAB_E_NOMEM (-3)
#define WAB_E_STATE (-4)      /* call not allowed in the handle's current state */

/* Game options, field-for-field `default_game_options` (wab_env.py:11-39).
 * Booleans are int32 0/1.  `None` options of the reference are spelled with the
 * *_random flags.  The last block are batched-surface extensions. */
typedef struct wab_config {
  double reward_per_turn;          /* 0 */
  double reward_for_being_killed;  /* -1 */
  double reward_for_starving;      /* -1 */
  double reward_for_finishing;     /* 1 */
  double reward_for_eating;        /* 0.1 */
  int32_t gatherer_only;           /* 0  (action table wab_env.py:149-159) */
  int32_t lookout_only;            /* 1  (action table wab_env.py:160-170; eat gate :302) */
  int32_t restrict_view;           /* 0  (masks wab_env.py:109-139, applied :344-357) */
  int32_t starting_role;           /* 1 */
  int32_t starting_role_random;    /* 1 <=> starting_role None (wab_env.py:598-599) */
  int32_t starting_food_random;    /* 1 <=> starting_food None (wab_env.py:596-597) */
  double starting_food;            /* 1.0 */
  int32_t max_turns;               /* 80 */
  int32_t height;                  /* 11, odd */
  int32_t width;                   /* 11, odd */
  int32_t max_berries_per_bush;    /* 200, <= 255 */
  double bush_power;               /* 100 (informational: the threshold table carries it) */
  int32_t turns_to_fill_food;      /* 8 */
  int32_t turns_to_empty_food;     /* 40 */
  int32_t wolf_spawn_margin;       /* 1 */
  double chance_wolf_on_square;    /* 0.001 (spawn test is u < chance/2, wab_env.py:573) */
  double wolf_chance_to_despawn;   /* 0.05 (keep test is u > chance, wab_env.py:263) */
  int32_t wolves;                  /* 1 */
  int32_t wolves_can_move;         /* 1 */
  int32_t god_mode;                /* 0 (hidden key, wab_env.py:292) */
  /* ---- batched-surface extensions ---- */
  int32_t autoreset;               /* 1: a done env is reset inside the same step call */
  int32_t plane_stride;            /* bytes per grid row in `planes` (>= height; 0 = height) */
  int32_t eaten_capacity;          /* eaten-tile log slots per env, <= 255
                                    * (0 = max_turns clamped to [1, 255]) */
  int32_t wolf_slots;              /* live-wolf slots per env: 8 (0 = 8), 16 or 32; a spawn
                                    * beyond them is dropped and counted (wolf_overflow) */
  /* T_k (k = 1..max_berries_per_bush): the smallest 53-bit U with
   * round((U * 2^-53) ** bush_power * max_berries_per_bush) >= k (wab_env.py:632-635).
   * Copied at wab_create.  NULL: wab_create computes it with wab_bush_thresholds (libm);
   * the Python host passes the table of the reference's own numpy arithmetic
   * (wab_gym_amd.options.bush_thresholds; the two agree on every option set tested). */
  const uint64_t* bush_thresholds;
} wab_config;

/* One observation batch — the reference's 7-tuple (wab_env.py:374-385) with a
 * leading batch dimension.  All device pointers, caller-owned.
 *   planes     [B][3][width][plane_stride] u8 0/1: wolf, bush, ostrich grids.
 *              Axis 1 is x, cell [width/2 + (ox - x)][height/2 + (oy - y)]
 *              (wab_env.py:403-409); padding bytes are written as 0.
 *   food_turns [B] u8  ceil(food * turns_to_empty_food)   (wab_env.py:450-452)
 *   role       [B] u8                                      (wab_env.py:390-391)
 *   status     [B] u8  0 alive, 1 starved, 2 killed        (wab_env.py:387-388)
 * view_mask (7th element) is a pure function of role and options; the host side
 * derives it (wab_env.py:360-368). */
typedef struct wab_obs {
  uint8_t* planes;
  uint8_t* food_turns;
  uint8_t* role;
  uint8_t* status;
} wab_obs;

/* Device-side counters, read back by wab_get_counters (synchronising). */
typedef struct wab_counters {
  uint64_t wolf_overflow;    /* wolves dropped because all wolf_slots slots were live */
  uint64_t eaten_overflow;   /* eats not logged because the eaten-tile log was full */
  uint64_t bad_actions;      /* actions outside [0, n_actions): treated as no-op */
  uint64_t steps;            /* env-steps executed: B per step-kernel launch (graph replays
                              * of captured wab_step calls included) */
  uint64_t resets;           /* env resets executed */
  uint64_t ego_missing;      /* wab_egocentric calls that found a turn of the path unrecorded */
  uint64_t handoff_timeouts; /* waits on an in-workgroup LDS hand-off that gave up (a hang
                              * guard; nonzero means results are invalid; must stay 0) */
  uint64_t wolf_overflow_reset; /* the part of wolf_overflow dropped by resets (a new episode's
                                 * initial wolves beyond the slots); the rest are ring spawns */
  uint64_t rollout_launches;   /* wab_rollout / wab_rollout_features / wab_rollout_policy calls that ran as ONE launch
                                * (host-side tally) */
  uint64_t rollout_step_calls; /* ... that ran as T per-step calls instead (misaligned plane
                                * slices, other kernels; host-side tally) */
} wab_counters;

typedef struct wab_handle wab_handle;

/* ABI version compiled into the library (== WAB_ABI_VERSION). */
int wab_abi_version(void);

/* Last error message of the calling thread ("" if none). */
const char* wab_last_error(void);

/* Number of actions of the table selected by the options (5 or 6, wab_env.py:149-182). */
int wab_num_actions(const wab_config* cfg);

/* The bush-value threshold table of wab_config.bush_thresholds, in C: out[k-1] = the
 * smallest U in [1, 2^53] with nearbyint(pow(U * 2^-53, bush_power) * max_berries) >= k
 * (generate_n_bush_values, wab_env.py:631-635; 2^53 = no draw reaches k), by bisection
 * over the 2^53 grid.  Host only, synchronous, no device needed. */
int wab_bush_thresholds(double bush_power, int32_t max_berries, uint64_t* out);

/* Validate options and allocate state for `batch` envs on HIP device `device`.
 * Env i has global id env_id_base + i; every random draw is keyed by
 * (seed, global id, episode, ...), so results do not depend on batch size, shard
 * count or device.  Synchronous.  No env is reset yet: call wab_reset first. */
int wab_create(const wab_config* cfg, int64_t batch, uint64_t seed, int64_t env_id_base,
               int device, wab_handle** out);

/* Free the handle and its device state (synchronises the device). */
int wab_destroy(wab_handle* h);

/* Reset envs (all, or those with mask[i] != 0; mask is a device pointer or NULL) and
 * write their observations into `obs` (other envs' obs entries are left untouched).
 * The first reset of an env is episode 0; each later reset increments its episode. */
int wab_reset(wab_handle* h, const uint8_t* mask, const wab_obs* obs, void* stream);

/* One step of every env.  actions: [B] int8 device.  Writes obs, reward [B] f32
 * (the reference's double reward rounded to f32), done [B] u8.
 * With cfg.autoreset, an env that is done is reset in the same call: `obs` then holds
 * the new episode's first observation and, if `terminal` is non-NULL, the step's own
 * observation is written to `terminal` (only the done envs' entries are written).
 * Without autoreset the env keeps stepping after done exactly as the reference does
 * (stepping after done is not guarded, wab_env.py:250). */
int wab_step(wab_handle* h, const int8_t* actions, const wab_obs* obs, float* reward,
             uint8_t* done, const wab_obs* terminal, void* stream);

/* T steps, stream-ordered, no host synchronisation.  actions [T][B] int8; obs planes
 * [T][B][3][width][plane_stride] and the scalar arrays [T][B] (an obs "sequence");
 * reward/done [T][B].  Bit for bit T calls of wab_step with terminal = NULL.  Where the small
 * or the wide kernel steps the handle (wab_step_kernel "small" / "wide") and B * width *
 * plane_stride * 3 is a multiple of 16, this is ONE launch: each workgroup takes its 64 envs
 * through the T steps with their state on chip (loaded by the first step, stored by the
 * last); otherwise T wab_step launches (a step slice that is not 16-byte aligned goes through
 * a handle-owned [B] buffer, allocated synchronously by the first such call, and a
 * device-to-device copy on `stream`). */
int wab_rollout(wab_handle* h, const int8_t* actions, int32_t T, const wab_obs* obs_seq,
                float* reward, uint8_t* done, void* stream);

/* Read the device counters (synchronises `stream`). */
int wab_get_counters(wab_handle* h, wab_counters* out, void* stream);

/* Copy hidden per-env state to HOST arrays (any may be NULL; synchronises `stream`):
 * food [B] f64, x/y [B] i32, turn [B] i32, n_wolves [B] i32, episode [B] u32. */
int wab_get_state(wab_handle* h, double* food, int32_t* x, int32_t* y, int32_t* turn,
                  int32_t* n_wolves, uint32_t* episode, void* stream);

/* Batch size of a handle. */
int64_t wab_batch(const wab_handle* h);

/* Where the caller's wab_step observations go, a performance hint with no effect on results
 * (default WAB_OBS_SAME_BUFFER):
 *   WAB_OBS_SAME_BUFFER   every step into the same obs buffer (the env's own, as
 *                         BatchedWolvesAndBushesEnv.step does): the per-step kernel, which stores
 *                         each plane as soon as it is final (a 128-byte line at a plane or env
 *                         boundary written in two parts, which the Infinity Cache merges when the
 *                         buffer stays resident);
 *   WAB_OBS_FRESH_BUFFER  each step into a buffer the last steps did not write (a closed loop's
 *                         ring of obs slots): on the wide kernel (wab_step_kernel "wide"), without
 *                         terminal obs, a one-step launch of its rollout build, which stores whole
 *                         lines in address order after the step (C3 at B = 65536: 52 us per step
 *                         into a 32-slot ring, against 73 us for the per-step kernel).
 * Other kernels ignore it.  Host only, no synchronisation. */
#define WAB_OBS_SAME_BUFFER 0
#define WAB_OBS_FRESH_BUFFER 1
int wab_set_obs_placement(wab_handle* h, int32_t placement);

/* Name of the kernel wab_step launches for this handle: "small" (the four-wave kernel for
 * views of at most 128 cells in unpadded rows), "wide" (width <= 31 and height <= 32, in rows
 * of 16 or 32 bytes, without restrict_view: the 31x31 configuration; width 32 steps on "block")
 * or "block" (the general one).  Diagnostics only. */
const char* wab_step_kernel(const wab_handle* h);

/* ---- config 5 (actor_critic.py rollout) ------------------------------------------ */

/* Length of the flattened PragmaticObsWrapper observation for the handle's options
 * (449 for the defaults), or WAB_E_INVALID if the wrapper cannot index the grids. */
int wab_feature_dim(const wab_handle* h);

/* PragmaticObsWrapper.observation (wab_env.py:726-824) + gym 0.17 spaces.flatten
 * (actor_critic.py:188) on device: obs -> features [B][F] float32 one-hot values.
 * view_mask: [B][11][11] u8 device pointer, or NULL to derive it from role and the
 * options as _get_obs does (wab_env.py:360-368). */
int wab_featurize(wab_handle* h, const wab_obs* obs, const uint8_t* view_mask, float* features,
                  void* stream);

/* wab_step fused with wab_featurize: PragmaticObsWrapper(WolvesAndBushesEnv).step
 * (actor_critic.py:180-192 wraps the env, so the policy only ever sees the features;
 * wab_env.py:670-824 applied to the obs of wab_env.py:250-342).  features [B][F] float32
 * (F = wab_feature_dim) are those of the obs this step returns (after auto-reset), bit for
 * bit what wab_step followed by wab_featurize(view_mask = NULL) would produce; reward, done
 * and the obs scalars are written as by wab_step.  No terminal obs.
 * obs->planes may be NULL: the planes are then not returned.  When the small-view kernel
 * steps the handle (wab_step_kernel == "small") and its views fit the table-driven
 * featurizer, one kernel does both (planes rendered on chip, stored only if asked for);
 * otherwise the call is wab_step then wab_featurize on `stream` (without caller planes
 * through a handle-owned buffer the first such call allocates, synchronously).
 * features (and planes, if set) must be 16-byte aligned. */
int wab_step_features(wab_handle* h, const int8_t* actions, const wab_obs* obs, float* reward,
                      uint8_t* done, float* features, void* stream);

/* T steps of PragmaticObsWrapper(WolvesAndBushesEnv).step with pre-chosen actions (the loop of
 * actor_critic.main, actor_critic.py:185-200) and, if `returns` is non-NULL, the discounted
 * returns of the segment (finish_episode, actor_critic.py:139-143): bit for bit T calls of
 * wab_step_features (actions [T][B]; obs_seq scalars [T][B], planes [T][B][3][width][stride]
 * or NULL; reward, done [T][B]; features [T][B][F]) followed by wab_discounted_returns_exact
 * over the [T][B] reward/done (R_T = bootstrap[b], NULL = 0; returns [T][B] f32).  Where the
 * fused small-view kernel steps the handle this is ONE launch: every workgroup takes its 64 envs
 * through the T steps with the state in registers, step t's feature rows stored while step
 * t + 1 runs, and (T <= 128) the returns computed from each step's exact double reward at the
 * end; elsewhere T wab_step_features calls and wab_discounted_returns_exact (misaligned plane
 * slices as in wab_rollout).  Every step's features must be 16-byte aligned: B * F a multiple
 * of 4.  With returns, T > 128 (or a non-fused handle) needs the exact-reward scan: when two of
 * the options' rewards round to the same float32 the call fails before any step runs. */
int wab_rollout_features(wab_handle* h, const int8_t* actions, int32_t T, const wab_obs* obs_seq,
                         float* reward, uint8_t* done, float* features, double gamma,
                         const float* bootstrap, float* returns, void* stream);

/* SuperBasicObservationWrapper.observation (wab_env.py:900-927) + gym flatten: the nearest
 * bush of the bush grid (4 x Discrete(max_distance)), food, role, status -> one-hot float32
 * [B][wab_superbasic_dim(h)] (90 for the defaults).  features must be 16-byte aligned. */
int wab_superbasic_dim(const wab_handle* h);
int wab_featurize_superbasic(wab_handle* h, const wab_obs* obs, float* features, void* stream);

/* WolvesAndBushesEnv.render(mode="rgb_array", scale, draw_health) (wab_env.py:468-502) of an
 * observation this handle produced: rgb [B][W*scale][H*scale][3] u8 device pointer.  With
 * draw_health != 0 (the reference's default) the turns-until-starve count (obs->food_turns)
 * is drawn at (0, 0) in blue with the digit glyphs of PIL's default font (wab_glyphs.h). */
int wab_render(wab_handle* h, const wab_obs* obs, int32_t scale, int32_t draw_health, uint8_t* rgb,
               void* stream);
/* The same for envs [first, first + count) of the observation only: rgb [count][W*scale]
 * [H*scale][3] (one env's frames for the Monitor's video recorder, gym.wrappers.Monitor
 * via wab_env.py:1013, actor_critic.py:46). */
int wab_render_envs(wab_handle* h, const wab_obs* obs, int64_t first, int64_t count, int32_t scale,
                    int32_t draw_health, uint8_t* rgb, void* stream);

/* Bush proximities of the egocentric env variants (WolvesAndBushesEnvEgoCentric and
 * WolvesAndBushesEnvEgocentricJustBushes, wab_env.py:930-979) for the handle's current state:
 * proximity u8 [B][5] (device), for the squares reached by up, right, down, left, stay:
 * clip(md - d, 0, md), d = taxicab distance to the nearest food>0 bush among every tile seen
 * this episode, md = width//2 + height//2 + 1 (<= 31 required); md for all five when no such
 * bush exists (wab_env.py:664).  mask (device u8 [B], nullable) limits the envs written.
 * The handle keeps a path of ostrich tiles for this: call it after EVERY wab_reset and
 * wab_step of the envs it observes (turn t's entry is written at turn t); a missing entry
 * counts in wab_counters.ego_missing.  Not valid after wab_rollout, nor after
 * wab_snapshot_restore (a snapshot does not hold the path). */
int wab_egocentric(wab_handle* h, const uint8_t* mask, uint8_t* proximity, void* stream);

/* Discounted returns of actor_critic.finish_episode (actor_critic.py:139-143) over a
 * [T][B] rollout: R_t = r_t + gamma * R_{t+1}, restarted after every done_t, R_T =
 * bootstrap[b] (NULL = 0).  Accumulated in double as the reference's Python floats are;
 * written as f32.  All pointers device. */
int wab_discounted_returns(const float* reward, const uint8_t* done, int32_t T, int64_t B,
                           double gamma, const float* bootstrap, float* returns, void* stream);

/* wab_discounted_returns over rewards that this handle's steps returned: each float32 reward
 * is first mapped back to the exact double the reference's step() returns (0 + r_x or
 * 0 + r_eat + r_x, wab_env.py:251-340; e.g. -0.8999999999999999 for 0.1 + -1, whose float32
 * is -0.9f), so the returns equal float32 of finish_episode's own double returns
 * (actor_critic.py:139-145) bit for bit.  Rewards outside that set are used as given.
 * WAB_E_INVALID if two of the options' rewards round to the same float32. */
int wab_discounted_returns_exact(const wab_handle* h, const float* reward, const uint8_t* done, int32_t T,
                                 int64_t B, double gamma, const float* bootstrap, float* returns,
                                 void* stream);

/* ---- per-episode statistics of a rollout segment ----------------------------------- */

/* Bytes of device workspace wab_episode_stats_update needs for a [T][B] segment (may be 0 for
 * T = 0), or WAB_E_INVALID (T < 0, B outside [1, 2^31), T * ceil(B / 64) >= 2^39). */
int64_t wab_episode_stats_workspace(int32_t T, int64_t B);

/* The episode returns and lengths gym.wrappers.Monitor keeps for the reference's training loop
 * (actor_critic.py:46, its "running reward" :210-224), over the reward f32 / done u8 [T][B] of a
 * rollout segment, for all B envs at once.  `ret` f64 [B] and `length` i64 [B] are the caller's
 * running state, read and written: for t = 0..T-1 in order, per env, ret += r, length += 1, and
 * where done[t][b] one finished episode (ret, length, env b, step t) is emitted and ret and
 * length restart at 0.  With a handle each float32 reward is first mapped to the exact double the
 * reference's step() returns (the table and rule of wab_discounted_returns_exact), so an
 * episode's return is the Monitor's own sum of Python floats bit for bit; with h = NULL rewards
 * are used as given.  The double adds of an env happen in step order.
 * The finished episodes are written compacted into ep_return f64, ep_length i32, ep_env i32 and
 * ep_step i32, each [capacity], in ascending (step, env) order; count i64 [2] receives
 * {finished, written}: when finished > capacity only the first `capacity` episodes of that order
 * are written and nothing past `capacity` is touched.  The four arrays may be NULL with
 * capacity 0 (count only).  workspace: wab_episode_stats_workspace(T, B) bytes, 8-byte aligned,
 * its contents meaningless before and after.  All pointers device; stream-ordered, no host
 * synchronisation, no atomics: the output is the same on every run.  T = 0 writes count = {0, 0}.
 * WAB_E_INVALID if two of the handle's rewards round to the same float32. */
int wab_episode_stats_update(const wab_handle* h, const float* reward, const uint8_t* done, int32_t T,
                             int64_t B, double* ret, int64_t* length, double* ep_return, int32_t* ep_length,
                             int32_t* ep_env, int32_t* ep_step, int64_t capacity, int64_t* count,
                             void* workspace, void* stream);

/* finish_episode's normalisation (actor_critic.py:145-146) per episode of a returns f32 / done u8
 * [T][B] segment: in every env's column a segment ends at each done, and one still open at step
 * T - 1 is normalised as it stands.  Per segment of n steps, in float64, sequential in step order:
 * mean = sum(x) / n, var = sum((x - mean)^2) / (n - 1) (torch.std is unbiased),
 * out = float32((x - mean) / (sqrt(var) + eps)); a one-step segment gives NaN, as torch.std does.
 * out f32 [T][B] may be `returns` itself.  All pointers device. */
int wab_normalize_episode_returns(const float* returns, const uint8_t* done, int32_t T, int64_t B, double eps,
                                  float* out, void* stream);

/* ---- advantages of a rollout segment ------------------------------------------------ */

/* Generalised advantage estimation over the reward f32 / done u8 / value f32 [T][B] of a rollout
 * segment, and the value targets advantage + value.  last_value [B] f32 is the critic's value of
 * the state after step T - 1 (NULL = 0).  Numeric contract (normative).  Per env b, in float64,
 * in this order, with no contraction:
 *
 *   gl = gamma * lambda                       (one double multiply, on the host)
 *   A = 0.0;  vnext = last_value ? (double)last_value[b] : 0.0
 *   for t = T-1 .. 0:
 *       v = (double)value[t][b]
 *       r = the step's exact double reward (the handle's table, as wab_discounted_returns_exact
 *           maps it; h == NULL: (double)reward)
 *       d = done[t][b] != 0                   (any nonzero byte)
 *       delta = (r + (d ? 0.0 : gamma * vnext)) - v
 *       A     = delta + (d ? 0.0 : gl * A)
 *       advantage[t][b] = (float)A;  target[t][b] = (float)(A + v)
 *       vnext = v
 *
 * The two selects are part of the contract, including what + 0.0 does to a -0.0.  NaN and
 * infinities propagate as the arithmetic says, up to the next done.  advantage, target [T][B] f32:
 * either may be NULL, not both.  Neither may overlap an input or the other (the scan reads
 * value[t] again as step t - 1's vnext): the host checks the byte ranges, WAB_E_INVALID.
 * WAB_E_INVALID too for T < 0, B < 0, a NULL required pointer, or a handle two of whose rewards
 * round to the same float32 (as wab_discounted_returns_exact), all before anything is launched.
 * T = 0 or B = 0 launches nothing.  All pointers device.  One launch, no allocation, no host
 * synchronisation, safe to capture in a hipGraph. */
int wab_gae(const wab_handle* h, const float* reward, const uint8_t* done, const float* value,
            const float* last_value, int32_t T, int64_t B, double gamma, double lambda, float* advantage,
            float* target, void* stream);

/* (x - mean) / (std + eps) over all n elements of x, the usual advantage normalisation over a
 * whole batch (the whole-tensor sibling of wab_normalize_episode_returns): mean = sum(x) / n,
 * var = sum((x - mean)^2) / (n - 1) (unbiased, as torch.std), out = float32((x - mean) /
 * (sqrt(var) + eps)), all in float64.  n = 1 gives NaN, n = 0 launches nothing.  The sums run in
 * an order that depends on n alone (per-workgroup partial sums in the workspace, then a combining
 * pass; no atomics): two runs on one input give the same bits.  out f32 [n] may be x itself,
 * else must not overlap it.  workspace: wab_whiten_workspace(n) bytes of device memory, 8-byte
 * aligned, its contents meaningless before and after; the size is WAB_E_INVALID for n < 0 or
 * n > 2^40, which wab_whiten refuses too.  Three stream-ordered launches, no allocation, no host
 * synchronisation, safe to capture in a hipGraph. */
int64_t wab_whiten_workspace(int64_t n);
int wab_whiten(const float* x, int64_t n, double eps, float* out, void* workspace, void* stream);

/* ---- snapshots: save and restore env state ---------------------------------------- */

/* A snapshot is one fixed-size record per env, env-major: env k of a snapshot is bytes
 * [k * R, (k + 1) * R) of `records`, R = wab_snapshot_bytes (a multiple of 16; 480 for the
 * defaults), so any env range is one contiguous slice.  A record holds everything an episode
 * needs to continue: the env's header (tile, turn, role / status / counts, episode), its food
 * (f64), wolf_slots wolf tiles, eaten_capacity eaten-log entries (tiles u32, then berries left
 * u8) and the bush bitmap of the view (bit i * height + j, after the eat).  It is canonical:
 * wolf slots, log entries and bitmap bits that are not live are 0, and the layout does not
 * depend on which step kernel runs the handle (wab_step_kernel), so equal states give equal
 * bytes and a snapshot moves between handles of any plane_stride.  Every draw is keyed by
 * (seed, global env id, episode, ...): a record restored into the slot with the same global id
 * continues bit for bit, in the same handle or another one, of any batch size.
 * Not in a snapshot: wab_counters (cumulative, left as they are), the caller's observation
 * buffers (the current observation is taken before the step's eat and spawn, so it cannot be
 * derived from a record: a caller that rewinds keeps its own copy), and the path of
 * wab_egocentric, which is not valid after a restore, as it is not after wab_rollout. */
#define WAB_SNAPSHOT_MAGIC 0x53424157u /* the bytes 'W' 'A' 'B' 'S' */
#define WAB_SNAPSHOT_VERSION 1u
typedef struct wab_snapshot_info {   /* host POD, describes a block of records */
  uint32_t magic, version;           /* WAB_SNAPSHOT_MAGIC, WAB_SNAPSHOT_VERSION */
  uint64_t config_hash;              /* wab_snapshot_hash of the saving handle's options */
  uint64_t seed;
  int64_t env_id_first, count;       /* global ids [first, first + count) */
  int64_t record_bytes;
} wab_snapshot_info;

/* R for these options (host only, no device needed); < 0 on options wab_create refuses. */
int wab_snapshot_bytes(const wab_config* cfg);

/* Hash of what decides how a state continues: every rule field, width, height, autoreset, the
 * resolved wolf_slots and eaten_capacity and the threshold table (NULL hashes as the table
 * wab_bush_thresholds gives).  Not plane_stride.  Host only; 0 on options wab_create refuses. */
uint64_t wab_snapshot_hash(const wab_config* cfg);

/* Write the records of envs [first, first + count) of the handle (indices into the handle) to
 * `records` (device, 16-byte aligned, count * R bytes) and describe them in `info`
 * (env_id_first = the handle's env_id_base + first).  One stream-ordered launch: no allocation,
 * no synchronisation.  WAB_E_STATE before the first wab_reset, WAB_E_INVALID for a range outside
 * [0, B). */
int wab_snapshot_save(wab_handle* h, int64_t first, int64_t count, void* records, wab_snapshot_info* info,
                      void* stream);

/* Env i of the handle, of global id g, takes record g - info->env_id_first when g lies in the
 * snapshot's id range and mask (device u8 [B], or NULL) is NULL or mask[i] != 0; every other env
 * is left untouched.  `records` is the snapshot's first record (device, 16-byte aligned).  One
 * stream-ordered launch; every range is checked on the host first.  WAB_E_INVALID (the message
 * names the check) when magic, version, config_hash, seed or record_bytes differ from the
 * handle's, or the two id ranges do not intersect.  A handle that was never reset accepts only a
 * restore of all its envs with mask = NULL, which then counts as its first wab_reset; any other
 * restore into it is WAB_E_STATE. */
int wab_snapshot_restore(wab_handle* h, const wab_snapshot_info* info, const void* records,
                         const uint8_t* mask, void* stream);

/* ---- device policy: the closed loop's action in one launch --------------------------- */

/* The actor-critic network of actor_critic.py:54-97 for inference: three Linear + leaky_relu
 * (slope 0.01) layers of widths h1, h2, h3, clamp(-4, 4) after the third, a softmax action head
 * (n_actions units) and a one-unit value head.  in_features >= 1, h1, h2, h3 in [1, 256],
 * n_actions in [2, 8]; the reference's net is {449, 128, 150, 128, 5}.
 * Numeric contract: every matmul operand (input features, weights, hidden activations after
 * bias, leaky_relu and clamp) is rounded to bf16, nearest even; products accumulate in fp32;
 * bias, activation, clamp, softmax (max-subtracted, expf, one divide) and the value are fp32.
 * Features that are 0 or 1, as wab_step_features writes them, are exact.  The reference's
 * + U(0, 1) / 100 input noise (actor_critic.py:189) is not reproduced.
 * Sampling: u = U * 2^-53 with U the 53-bit keyed draw of (seed, global env id, the env's current
 * episode, site 11, the env's current turn, tile (0, 0), k = 0), episode and turn read from the
 * handle's own state; action = #{k < n_actions - 1 : c_k <= u}, c_k the running sum in double,
 * k = 0, 1, ..., of the fp32 probabilities written to `probs`.  The action is an exact function
 * of probs and u, the same for any sharding of the batch.
 * Action rule (wab_policy_set_action_rule below; a fresh policy has {WAB_ACT_SAMPLE, 1.0f}, under
 * which every bit is as described above).  Temperature t: inv = 1.0f / t, computed on the host in
 * float32; in the head of wab_policy_act and wab_rollout_policy(_packed) logit_k is replaced by
 * lg'_k = fl32((logit_k + bias_k) * inv), rounded once (never contracted into the subtraction
 * that follows), and the softmax above is taken of lg': `probs` is the distribution the action is
 * taken from, `value` is untouched, and inv = 1.0f changes no bit.
 * WAB_ACT_SAMPLE: the keyed draw above on those probabilities.
 * WAB_ACT_GREEDY: a = 0, best = p_0; for k = 1 .. n_actions - 1: if (p_k > best) { best = p_k;
 * a = k; }, the p_k being the fp32 values written to `probs`: the first maximum of the
 * probabilities, ties to the lowest index, a row of NaNs gives action 0 (as sampling does); no
 * draw is made.  Like the sampled one, the action is an exact function of an output the caller
 * can see, the same for any sharding of the batch.
 * wab_policy_evaluate* and wab_policy_grad* (plain, _ppo, _gather, _packed) ignore the rule: they
 * are t = 1, bit for bit.  A caller who trains on rollouts made under t != 1 owns the importance
 * ratio: the behaviour log-probability of step's action a is log probs[a], not evaluate's logp. */
typedef struct wab_policy wab_policy;
typedef struct wab_policy_shape {
  int32_t in_features, h1, h2, h3, n_actions;
} wab_policy_shape;
/* fp32 device arrays in torch.nn.Linear's layout: weights [out][in], biases [out] (affine1,
 * affine2, affine3, action_head, value_head of actor_critic.Policy) */
typedef struct wab_policy_weights {
  const float *w1, *b1, *w2, *b2, *w3, *b3, *wa, *ba, *wv, *bv;
} wab_policy_weights;

/* Allocate the packed-weight image on `device` (synchronous).  WAB_E_INVALID for a shape outside
 * the ranges above. */
int wab_policy_create(const wab_policy_shape* shape, int device, wab_policy** out);

/* Round the weights to bf16 into the padded image the kernel reads: one stream-ordered launch, no
 * allocation, no synchronisation (a training loop reloads after every optimizer step). */
int wab_policy_load(wab_policy* p, const wab_policy_weights* weights, void* stream);

/* One launch: probs, value and the sampled action of every env of the handle from features
 * [B][in_features] float32 (e.g. those wab_step_features wrote; 4-byte aligned).  actions [B] int8;
 * probs [B][n_actions] float32 or NULL; value [B] float32 or NULL.  No host synchronisation, safe
 * to capture in a hipGraph.  WAB_E_INVALID when n_actions differs from the handle's or the policy
 * is on another device; WAB_E_STATE before the first wab_policy_load or the first wab_reset. */
int wab_policy_act(wab_handle* h, wab_policy* p, const float* features, int8_t* actions, float* probs,
                   float* value, void* stream);

/* Defined where the two entry points below exist (added without a change of WAB_ABI_VERSION:
 * nothing older changed). */
#define WAB_HAS_ACTION_RULE 1
enum { WAB_ACT_SAMPLE = 0, WAB_ACT_GREEDY = 1 };
typedef struct wab_action_rule {
  int32_t mode;      /* WAB_ACT_SAMPLE or WAB_ACT_GREEDY */
  float temperature; /* finite, > 0, with a finite, normal float32 reciprocal */
} wab_action_rule;

/* How wab_policy_act and wab_rollout_policy(_packed) choose the action (the numeric contract is
 * above).  Host state of the policy only: no device work, no stream, no allocation.  Every act
 * and rollout enqueued afterwards reads the rule as kernel arguments (the one-launch path and
 * the 2 T launches alike); work already enqueued, and a captured graph, keep the rule they were
 * enqueued or captured with.  wab_policy_load and wab_policy_adam_step leave it alone.
 * rule == NULL restores {WAB_ACT_SAMPLE, 1.0f}.  WAB_E_INVALID, the stored rule unchanged, for a
 * NULL policy, a mode that is neither of the two, a temperature that is not finite and > 0, or
 * one whose float32 reciprocal is zero, subnormal or infinite. */
int wab_policy_set_action_rule(wab_policy* p, const wab_action_rule* rule);

/* The rule as stored (the temperature as given).  WAB_E_INVALID for a NULL argument. */
int wab_policy_get_action_rule(const wab_policy* p, wab_action_rule* out);

/* Free the policy (synchronises its device). */
int wab_policy_destroy(wab_policy* p);

/* ---- device policy: the loss and its parameter gradients (actor_critic.py:148-165) ------ */

/* finish_episode()'s loss and loss.backward() over N stored rows, for the network wab_policy_load
 * last packed.  Per row i, with p = softmax(logits), H = -sum_k p_k log p_k:
 *   loss_policy  = -sum_i weight_i log p_i[a_i]     (weight: R - value.item(), or an advantage; a constant)
 *   loss_value   =  sum_i l(v_i - target_i)         (l: smooth_l1 with beta 1, or 0.5 d^2)
 *   loss_entropy =  sum_i H_i
 *   total        =  scale (loss_policy + value_coef loss_value - entropy_coef loss_entropy)
 * and the gradients of `total` with respect to the ten parameter tensors.
 * Numeric contract: the forward is wab_policy_act's (value has its bits).  The head is fp32.  The
 * backward pass is straight-through: every bf16 rounding of a weight, a feature or an activation
 * has derivative 1, so the gradient of the fp32 parameter is that of its rounded value.  Every
 * matrix product is bf16 x bf16 with fp32 accumulation: the gradient G_l of each layer's
 * pre-activation is rounded to bf16 before dW_l = G_l^T x_{l-1}, db_l = sum of the same rounded
 * rows, and dx_{l-1} = G_l bf16(W_l); leaky_relu passes 1 or float32(0.01) (z >= 0), the clamp 1
 * where -4 <= leaky_relu(z_3) <= 4 and 0 elsewhere.  Sums over rows have one fixed order that
 * does not depend on chunk_rows; no float atomics; results are bitwise reproducible. */
#define WAB_VALUE_LOSS_SMOOTH_L1 0
#define WAB_VALUE_LOSS_MSE 1
typedef struct wab_policy_loss {
  float value_coef;     /* 1 in the reference */
  float entropy_coef;   /* 0 in the reference */
  int32_t value_loss;   /* WAB_VALUE_LOSS_* */
  float scale;          /* multiplies `total` and every gradient, once, at the end (1 / N: a mean) */
  int32_t accumulate;   /* nonzero: add to grads_out and loss_out instead of overwriting them */
  int32_t chunk_rows;   /* rows per pass through the workspace: 0 = 32768, else a multiple of 128 */
} wab_policy_loss;

/* Bytes of workspace wab_policy_grad needs with this chunk_rows (it depends on the policy's shape
 * and chunk_rows, not on N); 0 with wab_last_error set for NULL, N outside [0, 2^31) or a
 * chunk_rows that is negative or no multiple of 128. */
size_t wab_policy_grad_workspace(const wab_policy* p, int64_t N, int32_t chunk_rows);

/* features [N][in_features] float32, actions [N] int8, weight [N] and target [N] float32;
 * grads_out: ten device arrays in wab_policy_weights' layout, written (or added to);
 * loss_out: device float[4] = {loss_policy, loss_value, loss_entropy, total} (the three parts
 * unscaled) or NULL; logp [N] (log p_i[a_i]), value [N], entropy [N] float32 or NULL.
 * workspace: device memory, 256-byte aligned, contents meaningless before and after.
 * Stream-ordered launches only (per chunk two, plus two): no allocation, no synchronisation,
 * safe to capture in a hipGraph.  N = 0 gives zero gradients and losses.
 * A row whose action is outside [0, n_actions) is left out of the losses and the gradients (its
 * logp is 0) and counted on the device; wab_policy_grad_bad_actions reports the count.
 * WAB_E_STATE before the first wab_policy_load; WAB_E_INVALID for a NULL required argument, N
 * outside [0, 2^31), a workspace smaller than wab_policy_grad_workspace's answer or misaligned,
 * a chunk_rows that is negative or no multiple of 128, or an unknown value_loss. */
int wab_policy_grad(wab_policy* p, const float* features, const int8_t* actions, const float* weight,
                    const float* target, int64_t N, const wab_policy_loss* loss,
                    const wab_policy_weights* grads_out, float loss_out[4], float* logp, float* value,
                    float* entropy, void* workspace, size_t workspace_bytes, void* stream);

/* The number of rows the latest wab_policy_grad on this workspace left out for their action
 * (synchronises `stream`).  WAB_E_INVALID, with the count in the message, when it is not 0. */
int wab_policy_grad_bad_actions(const wab_policy* p, const void* workspace, void* stream, uint64_t* out);

/* ---- device policy: PPO's clipped loss and the evaluate pass ---------------------------- */

/* wab_policy_grad with the clipped surrogate in the place of -weight logp, and optionally the
 * clipped value loss.  Per row i, everything not named here is wab_policy_grad's contract (forward,
 * p, log p_k, H, the entropy term, the straight-through backward, slabs, sum orders, scale once,
 * bad-action rows left out and counted).  A = advantage[i], fp32:
 *   d = logp_a - old_logp[i];  d = d < -30 ? -30 : (d > 30 ? 30 : d)   (a NaN stays a NaN)
 *   r = expf(d);  lo = 1.0f - clip, hi = 1.0f + clip, both formed in fp32
 *   clipped = (A > 0 && r > hi) || (A < 0 && r < lo)
 *   loss_policy_i = clipped ? -(A (A > 0 ? hi : lo)) : -(r A)
 *   w_eff = clipped ? 0 : r A   (one fp32 multiply)
 *   g_logit_k = w_eff (p_k - [k = a]) + entropy_coef p_k (log p_k + H)
 * which is -min(r A, clamp(r, lo, hi) A) and its gradient except on the ties.  Value term, l the
 * configured value loss, t the target, c = value_clip (c <= 0: off, old_value may be NULL):
 *   u = v - old_value[i];  |u| <= c: loss_value_i = l(v - t), g_v = value_coef l'(v - t)
 *   otherwise vc = old_value[i] + (u > 0 ? c : -c), l1 = l(v - t), l2 = l(vc - t),
 *   loss_value_i = max(l1, l2), value_clipped = l2 > l1, g_v = value_clipped ? 0 : value_coef l'(v - t)
 * ppo_out[4] = {clipped rows, sum of k3, value-clipped rows, sum of r} over the rows that took
 * part, k3 = expm1((double)d) - (double)d per row; summed in double in the loss parts' order, never
 * scaled.  With unchanged weights and old_logp from wab_policy_evaluate r is exactly 1.0f, and
 * the gradients are wab_policy_grad's of weight = advantage, bit for bit. */
typedef struct wab_ppo_config {
  float clip;         /* in (0, 1) */
  float value_clip;   /* <= 0: off */
} wab_ppo_config;

/* wab_policy_grad's arguments, guarantees and workspace, and: advantage [N], old_logp [N],
 * old_value [N] (NULL iff value_clip <= 0) float32; ppo_out: device float[4] or NULL, added to
 * with loss->accumulate as loss_out is; ratio [N] float32 or NULL (0 for a bad action).
 * WAB_E_INVALID also for a clip outside (0, 1) or NaN, a NULL old_logp with N > 0, or a NULL
 * old_value with value_clip > 0. */
int wab_policy_grad_ppo(wab_policy* p, const float* features, const int8_t* actions, const float* advantage,
                        const float* target, const float* old_logp, const float* old_value, int64_t N,
                        const wab_policy_loss* loss, const wab_ppo_config* ppo,
                        const wab_policy_weights* grads_out, float loss_out[4], float ppo_out[4],
                        float* logp, float* value, float* entropy, float* ratio,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Forward and head alone: logp [N] (log p_i[a_i]; 0 for a bad action, counted as in
 * wab_policy_grad), value [N] and entropy [N] float32 with the bits wab_policy_grad writes to its
 * row outputs (value: wab_policy_act's).  Each may be NULL; actions may be NULL when logp is.
 * workspace: wab_policy_grad's, or any 256-byte-aligned device memory of at least 256 bytes;
 * wab_policy_grad_bad_actions works on it after the call.  One memset node and one launch,
 * stream-ordered: no allocation, no synchronisation, safe to capture in a hipGraph. */
int wab_policy_evaluate(wab_policy* p, const float* features, const int8_t* actions, int64_t N,
                        float* logp, float* value, float* entropy,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- device policy: rows gathered by an index (PPO's shuffled minibatches) --------------- */

/* Defined where the four entry points below exist (they were added without a change of
 * WAB_ABI_VERSION: nothing older changed). */
#define WAB_HAS_POLICY_GATHER 1

/* wab_policy_grad, wab_policy_grad_ppo and wab_policy_evaluate with their rows taken through an
 * index: rows [N] int32 on the device, M the rows of the source.  Row i of the call takes every
 * input from source row rows[i]: features is [M][in_features], and actions, weight / advantage,
 * target, old_logp and old_value are [M].  The row outputs logp, value, entropy and ratio stay [N],
 * written at i (nothing is scattered).  The row blocks, the slabs and every sum order are those of
 * rows 0 .. N - 1, so each call is, bit for bit, its contiguous counterpart on gathered copies
 * (all ten gradients, loss_out, ppo_out and the row outputs).  An index may occur more than once,
 * and N may exceed M.  The index is read on the device at its place in the stream: a captured
 * graph replays correctly after a new permutation has been written into the same buffer.
 * An index outside [0, M) never becomes an address: it is clamped into [0, M - 1] before the
 * first load that uses it, and its row is treated as a bad-action row is (left out of every sum
 * and gradient, logp = ratio = 0, value and entropy those of the clamped source row) and counted
 * for wab_policy_grad_bad_rows; wab_policy_grad_bad_actions keeps counting bad actions only.
 * Launches, workspace and errors are the contiguous calls'; WAB_E_INVALID also for rows == NULL
 * with N > 0, M outside [1, 2^31) or a rows pointer that is not 4-byte aligned. */
int wab_policy_grad_gather(wab_policy* p, const float* features, const int8_t* actions, const float* weight,
                           const float* target, int64_t N, const wab_policy_loss* loss,
                           const wab_policy_weights* grads_out, float loss_out[4], float* logp, float* value,
                           float* entropy, void* workspace, size_t workspace_bytes, void* stream,
                           const int32_t* rows, int64_t M);
int wab_policy_grad_ppo_gather(wab_policy* p, const float* features, const int8_t* actions, const float* advantage,
                               const float* target, const float* old_logp, const float* old_value, int64_t N,
                               const wab_policy_loss* loss, const wab_ppo_config* ppo,
                               const wab_policy_weights* grads_out, float loss_out[4], float ppo_out[4],
                               float* logp, float* value, float* entropy, float* ratio,
                               void* workspace, size_t workspace_bytes, void* stream,
                               const int32_t* rows, int64_t M);
int wab_policy_evaluate_gather(wab_policy* p, const float* features, const int8_t* actions, int64_t N,
                               float* logp, float* value, float* entropy,
                               void* workspace, size_t workspace_bytes, void* stream,
                               const int32_t* rows, int64_t M);

/* The number of rows the latest call on this workspace left out for their index (synchronises
 * `stream`; 0 after a contiguous call).  WAB_E_INVALID, with the count in the message, when it is
 * not 0. */
int wab_policy_grad_bad_rows(const wab_policy* p, const void* workspace, void* stream, uint64_t* out);

/* ---- packed feature rows: 1 bit per feature ------------------------------------------------ */

/* Defined where the entry points below exist (added without a change of WAB_ABI_VERSION: nothing
 * older changed).
 * The format.  A PragmaticObsWrapper row is a one-hot layout: every float is 0.0 or 1.0.  A packed
 * row of F features is P = 4 * ceil(F / 128) little-endian dwords (a multiple of 16 bytes):
 * feature k is bit (k & 31) of dword (k >> 5).  Every producer writes bits F .. 32 P - 1 as 0;
 * every consumer ignores them.  Arrays are [rows][P] uint32, 16-byte aligned.  The calls that read
 * packed rows give, bit for bit, the results of their float counterparts on the unpacked rows:
 * 0 and 1 are exact in bf16 and no sum changes its order. */
#define WAB_HAS_PACKED_FEATURES 1

/* P for rows of in_features features; WAB_E_INVALID outside wab_policy_create's range [1, 2^20]. */
int wab_feature_bits_pitch(int32_t in_features);

/* features [n_rows][F] float32 (4-byte aligned) -> bits [n_rows][P] (16-byte aligned): the bit is
 * set iff the float's bit pattern is not 0x00000000.  nonbinary (device, 8-byte aligned, or NULL):
 * the call adds the number of elements whose pattern is neither 0x00000000 nor 0x3F800000 (-0.0f
 * and NaN count).  wab_features_unpack writes exactly 0.0f or 1.0f.  Each is one launch on
 * `stream` (none when n_rows == 0), with no allocation and no synchronisation, safe to capture in
 * a hipGraph.  WAB_E_INVALID for a NULL or misaligned pointer with n_rows > 0, n_rows < 0, or F
 * outside [1, 2^20]. */
int wab_features_pack(const float* features, int64_t n_rows, int32_t F, uint32_t* bits, uint64_t* nonbinary,
                      void* stream);
int wab_features_unpack(const uint32_t* bits, int64_t n_rows, int32_t F, float* features, void* stream);

/* wab_policy_evaluate_gather, wab_policy_grad_gather and wab_policy_grad_ppo_gather with the
 * source's feature rows packed: feature_bits [M][P] (rows == NULL: [N][P]) in place of features.
 * rows == NULL means the contiguous rows 0 .. N - 1, and M is ignored; rows != NULL is the gather
 * contract unchanged (clamping, bad rows, the index read on the device).  Workspace, launches,
 * graph safety, bad-action counting and every refusal are the float calls'; feature_bits must be
 * 16-byte aligned. */
int wab_policy_evaluate_packed(wab_policy* p, const uint32_t* feature_bits, const int8_t* actions, int64_t N,
                               float* logp, float* value, float* entropy,
                               void* workspace, size_t workspace_bytes, void* stream,
                               const int32_t* rows, int64_t M);
int wab_policy_grad_packed(wab_policy* p, const uint32_t* feature_bits, const int8_t* actions, const float* weight,
                           const float* target, int64_t N, const wab_policy_loss* loss,
                           const wab_policy_weights* grads_out, float loss_out[4], float* logp, float* value,
                           float* entropy, void* workspace, size_t workspace_bytes, void* stream,
                           const int32_t* rows, int64_t M);
int wab_policy_grad_ppo_packed(wab_policy* p, const uint32_t* feature_bits, const int8_t* actions, const float* advantage,
                               const float* target, const float* old_logp, const float* old_value, int64_t N,
                               const wab_policy_loss* loss, const wab_ppo_config* ppo,
                               const wab_policy_weights* grads_out, float loss_out[4], float ppo_out[4],
                               float* logp, float* value, float* entropy, float* ratio,
                               void* workspace, size_t workspace_bytes, void* stream,
                               const int32_t* rows, int64_t M);

/* ---- device policy: the optimizer step (actor_critic.py:104, 165) ----------------------- */

/* torch.optim.Adam's step (AdamW's with `decoupled`) over the ten parameter tensors, with a
 * global-norm clip (torch's clip_grad_norm_ rule) and no step at all on a non-finite gradient
 * (the two guards actor_critic.py:112-113 asks for), and the re-pack of the bf16 image
 * wab_policy_act reads: after the call no wab_policy_load is needed.
 *
 * Numeric contract.  Flat order: the ten tensors in wab_policy_weights' order, each row-major; P
 * elements in all.  No operation is contracted into an fma; every operation named is IEEE
 * correctly rounded, round to nearest even.
 *   Norm:   q_i = (double)g_i * (double)g_i (exact);  S = the adjacent-pair tree sum of q,
 *           zero-padded to the next power of two >= P (x'[i] = x[2i] + x[2i+1] until one value is
 *           left);  norm = sqrt(S) in double;  grad_norm = (float)norm.
 *   Skip:   S not finite (some g_i is NaN or +-Inf): params, moments, the image, step and the
 *           beta powers keep their bits; skipped += 1; grad_norm and clip_scale are still written.
 *   Clip:   c = 1.0f if max_grad_norm <= 0, else with r = max_grad_norm / (norm + 1e-6) in
 *           double, c = (float)(r < 1.0 ? r : 1.0) (a NaN norm gives 1).  clip_scale = c.
 *   Scalars (double unless cast):
 *           b1p = (step == 0 ? 1.0 : beta1_pow) * beta1;  b2p likewise;
 *           a = (float)(lr / (1.0 - b1p));  r2 = sqrtf((float)(1.0 - b2p));
 *           b1f = (float)beta1, omb1 = (float)(1.0 - beta1), b2f, omb2 likewise, epsf = (float)eps,
 *           wdf = (float)weight_decay, decayf = (float)(1.0 - lr * weight_decay);
 *           then step += 1 and beta1_pow = b1p, beta2_pow = b2p are stored.  The beta powers are
 *           running products, so that they are the same bits everywhere (pow() is not).
 *   Per element, float32, in this order:
 *           g = g_i * c
 *           weight_decay != 0, not decoupled:  g = g + wdf * p
 *           weight_decay != 0, decoupled:      p = p * decayf
 *           m = b1f * m + omb1 * g
 *           v = b2f * v + (omb2 * g) * g
 *           den = sqrtf(v) / r2 + epsf
 *           p = p - a * (m / den)
 *           the image's element of p = bf16(p), nearest even, as wab_policy_load rounds it.
 * Results are bitwise reproducible: no atomics, every sum has one order, a function of the shape.
 * This is Adam as torch computes it up to the order of float32 roundings (torch: step_size / bias
 * corrections folded differently); DESIGN.md has both measured against float64. */
typedef struct wab_adam_config {   /* host, by pointer */
  double lr, beta1, beta2, eps, weight_decay;
  double max_grad_norm;            /* <= 0: no clip */
  int32_t decoupled;               /* nonzero: AdamW's decay */
} wab_adam_config;

typedef struct wab_adam_state {    /* DEVICE memory, caller-owned, 8-byte aligned; all-zero bytes = a fresh optimizer */
  uint64_t step, skipped;          /* steps taken; calls skipped for a non-finite gradient */
  double beta1_pow, beta2_pow;     /* beta^step as running products (read only when step > 0) */
  float grad_norm, clip_scale;     /* of the latest call */
  uint64_t reserved;
} wab_adam_state;

/* Bytes of workspace wab_policy_adam_step needs (it depends on the policy's shape alone); 0 with
 * wab_last_error set for NULL. */
size_t wab_policy_adam_workspace(const wab_policy* p);

/* params, exp_avg, exp_avg_sq: ten device arrays each in wab_policy_weights' layout, read and
 * written through (the const of the struct's fields notwithstanding, as wab_policy_grad's
 * grads_out); grads: read.  No array may overlap another.  state: device.  workspace: device
 * memory, 8-byte aligned, contents meaningless before and after.
 * Three stream-ordered launches (four where the network has more than 2^20 parameters): no
 * allocation, no synchronisation, safe to capture in a hipGraph; cfg is read on the host at the
 * call (a captured graph keeps its values).
 * The image's padding must already be zero, as wab_policy_load leaves it: WAB_E_STATE before the
 * first wab_policy_load.  WAB_E_INVALID, before anything is launched, for a NULL argument or
 * array pointer, lr < 0, a beta outside [0, 1), eps <= 0, weight_decay < 0, a NaN among them, a
 * workspace smaller than wab_policy_adam_workspace's answer, or a misaligned array, state or
 * workspace. */
int wab_policy_adam_step(wab_policy* p, const wab_policy_weights* params, const wab_policy_weights* grads,
                         const wab_policy_weights* exp_avg, const wab_policy_weights* exp_avg_sq,
                         const wab_adam_config* cfg, wab_adam_state* state, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- closed-loop rollout: policy and env step, T steps (actor_critic.py:108-125, 185-200) -- */

/* 1 when wab_rollout_policy(h, p, ...) runs as one launch, 0 when it runs as 2 T launches;
 * host only, no device work.  Negative WAB_E_* for NULL or a policy of another device.
 * One launch needs: the small-view kernel at the 11x11 geometry with 8 wolf slots and its fused
 * featurizer (the default options and any other rules at that geometry); a policy whose
 * in_features is wab_feature_dim(h) (every width wab_policy_create accepts is fused);
 * batch * feature_dim a multiple of 4; and the
 * kernel's LDS (the step's, a 128-step returns scan's, and the policy's bf16 images of 64 envs)
 * within the device's limit per workgroup.  The answer is for calls without planes; a call
 * with obs_seq->planes also needs batch * 3 * W * S to be a multiple of 16 and otherwise runs as
 * the 2 T launches. */
int wab_rollout_policy_fused(const wab_handle* h, const wab_policy* p);

/* T closed-loop steps.  The call equals, bit for bit, for t = 0 .. T-1:
 *   wab_policy_act(h, p, t == 0 ? features0 : features[t], actions[t], probs[t], value[t]);
 *   wab_step_features(h, actions[t], obs_seq[t], reward[t], done[t],
 *                     t + 1 < T ? features[t + 1] : features_last);
 * after which slice 0 of `features` holds features0 (features == features0 is allowed) and, if
 * `returns` is non-NULL, wab_discounted_returns_exact has run over the [T][B] reward / done with
 * `bootstrap` (as in wab_rollout_features: in the launch for T <= 128, the same refusal when two
 * of the options' rewards round to one float32).
 * features0 [B][F] float32, 4-byte aligned, any values (rounded to bf16 as wab_policy_act rounds
 * them); obs_seq scalars [T][B], planes [T][B][3][W][S] or NULL; actions [T][B] int8; value
 * [T][B], probs [T][B][n_actions], features [T][B][F] and returns [T][B] float32 or NULL;
 * reward [T][B] float32, done [T][B] uint8 and features_last [B][F] float32 are required;
 * features and features_last 16-byte aligned; features_last may be features0 (a continuing
 * rollout keeps one row array).  Where the answer is 0, wab_last_error() says which condition
 * failed.  With features == NULL the intermediate feature
 * rows are never written to device memory.
 * Where wab_rollout_policy_fused is 1 the call is one launch (each workgroup takes its 64 envs
 * through the T steps, the policy between them on the feature bits still on chip, the draw keyed
 * by the env's episode and turn after the step), with no allocation and no synchronisation, safe
 * to capture in a hipGraph.  Elsewhere it is the 2 T calls above on `stream`; with features ==
 * NULL, or feature slices that are not 16-byte aligned, that path goes through a handle-owned
 * pair of feature rows, which the first such call allocates (hipMalloc: make one such call
 * before capturing a graph; freed by wab_destroy).
 * wab_counters.steps and the resets advance as under the two calls; bad_actions stays 0.
 * WAB_E_STATE before the first wab_policy_load or wab_reset; WAB_E_INVALID for another n_actions
 * or in_features than the handle's, a policy on another device, a NULL required argument, or
 * misaligned features. */
int wab_rollout_policy(wab_handle* h, wab_policy* p, const float* features0, int32_t T,
                       const wab_obs* obs_seq, int8_t* actions, float* value, float* probs,
                       float* reward, uint8_t* done, float* features, float* features_last,
                       double gamma, const float* bootstrap, float* returns, void* stream);

/* wab_rollout_policy with the [T][B][F] float `features` replaced by feature_bits [T][B][P]
 * (WAB_HAS_PACKED_FEATURES; required, 16-byte aligned): slice t is wab_features_pack of what
 * features[t] would have held, slice 0 that of features0.  Everything else is wab_rollout_policy's,
 * bit for bit: features0 and features_last stay float32 [B][F]; actions, value, probs, reward,
 * done, returns, the counters and the refusals are unchanged.  Slice 0 is written by a
 * wab_features_pack launch queued in front on the same stream.  Where wab_rollout_policy_fused
 * is 1 the steps are then one launch, whose rows-out phase writes the packed rows from the
 * feature bits on chip (no float row reaches device memory but features_last); elsewhere each
 * step of the 2 T calls goes through the handle-owned pair of float rows and is followed by one
 * wab_features_pack launch into slice t + 1.  WAB_E_INVALID also for feature_bits == NULL or not
 * 16-byte aligned. */
int wab_rollout_policy_packed(wab_handle* h, wab_policy* p, const float* features0, int32_t T,
                              const wab_obs* obs_seq, int8_t* actions, float* value, float* probs,
                              float* reward, uint8_t* done, uint32_t* feature_bits, float* features_last,
                              double gamma, const float* bootstrap, float* returns, void* stream);

/* Test hook: the bush value (berries, generate_n_bush_values wab_env.py:631-635) the step
 * kernels give the 53-bit draws U[n] under h's threshold table, computed by the kernels' own
 * bracketed search (bush_value_fast).  U, out device pointers. */
int wab_debug_bush_values(wab_handle* h, const uint64_t* U, int32_t* out, int64_t n, void* stream);

/* Test hook: which instance of the returns scan wab_discounted_returns (h == NULL) or
 * wab_discounted_returns_exact (h) launches for these pointers and this B: out = {VEC, NE}.  VEC,
 * the envs per thread, is 4, else 2, else 1: the widest with B % VEC == 0, B / VEC >= 65536,
 * reward and returns aligned to 4 VEC bytes and done to VEC bytes.  NE is the number of the
 * handle's step rewards whose float32 is not their double (0 without a handle), 5 to 7 padded
 * to 8.  The launch takes its instance from the same host function.  Host only: launches
 * nothing, reads no device memory.  WAB_E_INVALID where wab_discounted_returns_exact refuses
 * the handle. */
int wab_debug_returns_plan(const wab_handle* h, const float* reward, const uint8_t* done, const float* returns,
                           int64_t B, int32_t out[2]);

/* Test hook: which instance of the GAE scan wab_gae launches for these pointers (advantage or
 * target may be NULL as in the call) and this B: out = {VEC, NE}.  VEC, the envs per thread, is 2
 * when B % 2 == 0, B / 2 >= 65536, reward, value and the outputs are 8-byte aligned and done is
 * 2-byte aligned, else 1.  NE as in wab_debug_returns_plan.  The launch takes its instance from
 * the same host function.  Host only: launches nothing, reads no device memory.  WAB_E_INVALID
 * where wab_gae refuses the handle. */
int wab_debug_gae_plan(const wab_handle* h, const float* reward, const uint8_t* done, const float* value,
                       const float* advantage, const float* target, int64_t B, int32_t out[2]);

/* Test hook: how wab_policy_act runs this policy: out = {input chunks of layer 1, columns per
 * chunk, columns of the last chunk, LDS bytes per workgroup, 1 for the instance with two
 * layer-1 tiles per wave (h1 > 128) or 0}.  Host only. */
int wab_debug_policy_plan(const wab_policy* p, int32_t out[5]);

/* Test hook: how wab_policy_grad runs this policy with this chunk_rows: out = {rows per row block,
 * slabs, rows per chunk, LDS bytes per workgroup of wab_policy_bwd_kernel, of
 * wab_policy_wgrad_kernel}.  Host only. */
int wab_debug_policy_grad_plan(const wab_policy* p, int32_t chunk_rows, int32_t out[5]);

#ifdef __cplusplus
}
#endif
#endif /* WAB_H_ */
