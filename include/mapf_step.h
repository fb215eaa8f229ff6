/*
 * mapf_step.h -- C ABI of libmapfstep.so, the MI355X (gfx950) vectorized step engine that replaces
 * the hot path of the reference's multi-agent grid environment
 * (/root/reference/src/environments/reference_model_multi_agent.py, "MA-env" below).
 *
 * One handle owns B independent env instances resident in HBM on one GPU.  Plain pointers and sizes
 * only; no torch / C++ types cross this boundary.  A handle is NOT thread-safe (the reference env is
 * single-threaded and not re-entrant either); use one handle per host thread / per GPU.
 *
 * Pointer convention
 *   - "host"   : ordinary host memory, copied synchronously inside the call (setup / inspection calls)
 *   - "device" : HIP device memory on the handle's GPU, caller-owned, used asynchronously on `stream`
 *                (the hot-path calls mapf_reset / mapf_step).  `stream` is a hipStream_t passed as void*
 *                (NULL = the default stream).  Every device pointer must be aligned to 16 bytes (observation rows leave in
 *                16-byte pieces); nothing more is assumed -- in particular not the 256 / 512 bytes of an allocator.
 *
 * Write contract of the device outputs.  A call stores to the elements listed for it and to no other byte: not to padding
 * behind a buffer, not to a row past [B], not to a slab past [T].  "Written" means every element is stored by the call,
 * whatever the buffer held before; "left alone" means not one byte of it is stored, so a caller may keep other data
 * there.  tests/test_output_contract_gpu.py holds every entry point to this on guarded, poisoned buffers.
 *
 * Every function returns MAPF_OK (0) or a negative MAPF_ERR_* code; mapf_last_error() gives the text.
 * Errors the reference raises as Python exceptions *inside* step() (bad action -> ValueError MA-env:504-506,
 * no respawn cell -> RuntimeError MA-env:296-298) happen per env on the device; they are latched in a
 * device-side error record that mapf_poll_error() reads back.
 *
 * Reference interface each entry point replaces (a maintainer binds these with ctypes):
 *   mapf_create + mapf_set_grids + mapf_set_rng_state (+ mapf_set_fixed_starts_goals)
 *                         <- ReferenceModel.__init__            MA-env:34-184 (config keys :38-61, state block :82-120,
 *                                                               RNG :74-78, grid :80, fixed tables :124-132)
 *   mapf_reset            <- ReferenceModel.reset               MA-env:440-472 (+ generate_starts_goals :267-282)
 *   mapf_step             <- ReferenceModel.step                MA-env:474-695 (+ get_obs :707-747, get_action_mask :749-773,
 *                                                               _flatten_observation :306-328, _assign_new_goal :284-304,
 *                                                               lock detector :374-438)
 *   mapf_get_state / mapf_set_state
 *                         <- the private arrays callers and tests read or poke: _positions_arr, _goals_arr, _starts_arr,
 *                            _reached_arr, _completed_once_arr, _blocking_pressure_prev_arr, step_count, _episode_* counters
 *                            (MA-env:83-89, :63-69; read by src/trainers/callbacks.py:111-131,265-307 and main.py:265,314)
 *   mapf_step_many        <- T x step() (+ reset() on done) for an action stream known up front: the loop of
 *                                                               scripts/benchmark_multi_agent_env.py:85-95
 *   mapf_get_episode_stats, mapf_episode_stats_async
 *                         <- what ReferenceModelCallbacks.on_episode_end reads from the env   src/trainers/callbacks.py:236-345
 *   mapf_observe          <- get_obs / get_action_mask / _flatten_observation called on a static state
 *                                                               MA-env:707-773, :306-328
 *   mapf_obs_len          <- _build_obs_layout                  MA-env:238-265
 *   mapf_assign_new_goal  <- _assign_new_goal(agent_idx) called by itself (the reference's lifelong tests do,
 *                            tests/test_reference_model_lifelong.py:132-173)                     MA-env:284-304
 *   mapf_render           <- render(mode="rgb_array")  MA-env:775-916 (an exact integer raster, not matplotlib's pixels)
 *   mapf_eval_begin / mapf_eval_record / mapf_eval_end
 *                         <- what the test mode keeps around its step loop: the per-episode result rows and the occupancy
 *                            heatmap                                                            main.py:153-155, :232-324
 *   mapf_cte_eval_begin / mapf_cte_eval_record
 *                         <- the same loop for the single-agent env (the reference's test mode has none: main.py:37)
 *   mapf_eval_trace_begin / mapf_eval_trace, mapf_render_words
 *                         <- the video of the first test episodes (SAVE_VIDEO)  main.py:49-53, :188-194, :239-243, :269-274
 *                            and the per-agent paths scripts/a-star.py:204-249 prints and measures: per-step state of
 *                            chosen envs of an evaluation, and frames redrawn from it
 *   mapf_expert_actions / mapf_path_lengths / mapf_distance_field
 *                         <- the classical baselines the reference compares its policies against (scripts/a-star.py: one
 *                            host search per agent): shortest-path expert, path-length lower bounds, per-goal distance maps
 *   mapf_observe_guided   <- (no counterpart) the same search as six floats in the observation: which moves shorten the path
 *   mapf_plan_prioritized <- the coordinated baseline (scripts/cbs.py plans the agents together; its result files hold
 *                            max_steps and agent_i_steps of a joint plan): prioritised planning in the env's move order
 *   mapf_plan_windowed    <- the same baseline for lifelong mode, where goals change under a plan
 *                            (tests/test_reference_model_lifelong.py): the next `window` steps planned together, replanned
 *                            as the window is played
 *   mapf_plan_cbs         <- scripts/cbs.py itself: conflict-based search, the optimal joint plan per env within a node
 *                            budget (our own rule, stated above the call; nothing of the script's is taken over)
 */
#ifndef MAPF_STEP_H
#define MAPF_STEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAPF_VERSION_MAJOR 0
#define MAPF_VERSION_MINOR 1

/* limits of this build (checked by mapf_create) */
#define MAPF_MAX_DIM 64          /* grid height and width */
#define MAPF_MAX_AGENTS 64       /* agents per env (one wavefront lane per agent) */
#define MAPF_MAX_SENSOR_RANGE 5  /* view side 2*sr+1 <= 11 */
#define MAPF_MAX_LOCK_WINDOW 64  /* deadlock / livelock window steps */
#define MAPF_RENDER_MIN_CELL_PX 4   /* mapf_render: pixels per grid cell */
#define MAPF_RENDER_MAX_CELL_PX 64
#define MAPF_PLAN_MAX_HORIZON(H) 256 /* mapf_plan_prioritized: planned steps, for every grid height H <= MAPF_MAX_DIM */
#define MAPF_CBS_MAX_HORIZON 128      /* mapf_plan_cbs: planned steps (a constraint's time takes 8 bits of a node's entry) */
#define MAPF_CBS_MAX_NODES 1024      /* mapf_plan_cbs: nodes per env (a node id takes 10 bits of an entry; the node tables, 12 bytes
                                        per node, bind the LDS of an env: see the call) */
#define MAPF_PLAN_MAX_WINDOW 64      /* mapf_plan_windowed: planned steps per call (history and cells of an env fit in LDS) */

/* config flags (defaults of the reference in brackets, MA-env:41-61) */
#define MAPF_FLAG_NORMALIZE_GOAL_DELTA 1u /* normalize_goal_delta [on]  */
#define MAPF_FLAG_GOAL_DISTANCE 2u        /* include_goal_distance [off] */
#define MAPF_FLAG_ACTION_MASK 4u          /* include_action_mask_in_obs [off] */
#define MAPF_FLAG_BLOCKING_PRESSURE 8u    /* include_blocking_pressure_in_obs [on] */
#define MAPF_FLAG_LIFELONG 16u            /* lifelong_mapf [off] */
#define MAPF_FLAG_LOCK_METRICS 32u        /* enable_lock_metrics [on] */
#define MAPF_FLAG_DETERMINISTIC 64u       /* deterministic [off]: reset() re-places agents on fixed starts, no RNG */
#define MAPF_FLAG_DERIVED_DISTANCE 128u    /* derived_distance_history [off]: a finite handle (no MAPF_FLAG_LIFELONG) whose lock windows
                                            * are both <= 16 steps keeps one bit per step instead of the 16 goal-distance bytes: 16
                                            * state bytes per agent instead of 32, same outputs (mapf_state_bytes_per_agent has the
                                            * details and the escape).  Ignored by every other handle. */
#define MAPF_FLAG_SINGLE_AGENT 256u        /* the handle runs the single-agent (CTE) sibling env: use the mapf_cte_* calls */
#define MAPF_FLAG_JIT_SPECIALIZE 0x10000000u /* opt-in: when no prebuilt specialisation of the step kernels matches, compile
                                               one for exactly this configuration at mapf_create (hiprtc, a few seconds;
                                               cached per process).  Falls back to the runtime-config kernels -- with the
                                               reason in mapf_jit_status() -- when hiprtc or the kernel source is not there */
#define MAPF_FLAG_FORCE_DENSE 0x08000000u   /* engine knob (tests): the 128-register builds of the small-group step kernels
                                             * whatever the size of the grid (mapf_create picks by grid size otherwise) */
#define MAPF_FLAG_FORCE_SPARSE 0x04000000u  /* engine knob (tests): never the 128-register builds */
#define MAPF_FLAG_SAMPLER_WORKGROUPS 0x02000000u /* engine knob (tests): the runtime-config kernels pre-draw placements in
                                             * sampler workgroups of the step grid instead of slices inside the env workgroups */
#define MAPF_FLAG_TWO_WAVE_WIDE 0x00800000u /* engine knob (tests / A-B): 64-lane groups step on the two-wave kernel with the
                                             * word-per-cell LDS map (rounds 1-3) instead of the three-wave kernel with bit rows */
#define MAPF_FLAG_TABLE_WALK_OBS 0x00400000u /* engine knob (tests / A-B): the observation wave of the three-wave small-group
                                             * kernel walks the agent table after the moves (round 3) instead of preparing
                                             * both outcomes of its agent's move from bit rows before them (round 4) */
#define MAPF_FLAG_NO_BIT_ROWS 0x00200000u /* engine knob (tests / A-B): the three-wave small-group kernel as of round 3 -- no
                                           * goal / occupancy / intent bit rows, per-agent outputs by the aux wave */
#define MAPF_FLAG_SEQUENTIAL_RESET 0x20000000u /* engine knob (tests): in-kernel resets always take the sequential
                                                 * sampler (otherwise only after a Lemire rejection or when F = 2N) */
#define MAPF_FLAG_NO_CELL_MAP 0x40000000u   /* engine knob (tests / A-B): never use the LDS cell-map path of wide groups */
#define MAPF_FLAG_GENERIC_KERNEL 0x80000000u /* engine knob (tests): never pick a compile-time specialised step kernel */

/* status codes */
#define MAPF_OK 0
#define MAPF_ERR_BAD_ACTION (-1)  /* reference: ValueError "Invalid action ..." MA-env:504-506 */
#define MAPF_ERR_FEW_FREE (-2)    /* reference: ValueError, fewer than 2N free cells MA-env:270-275 */
#define MAPF_ERR_NO_RESPAWN (-3)  /* reference: RuntimeError, no cell for lifelong goal MA-env:296-298 */
#define MAPF_ERR_CONFIG (-4)      /* config outside this build's limits / inconsistent arguments */
#define MAPF_ERR_HIP (-5)         /* a HIP runtime call failed */
#define MAPF_ERR_STATE (-6)       /* call sequence error (e.g. step before grids were set) */
#define MAPF_ERR_INTERNAL (-8)    /* checking build only (-DMAPF_CHECK): an index left the LDS region it belongs to; env, site
                                   * id and the offending value are latched like the device errors above */
#define MAPF_ERR_RNG_GUARD (-7)   /* device: a bounded draw was rejected 4096 times in a row (cannot happen with a sound
                                   * stream state, p < 1e-24000): the env's RNG state is corrupt; latched like the others */

/* info_all[...] column order: the reference's info["__all__"] keys MA-env:639-655 */
#define MAPF_INFO_ALL 14
#define MAPF_INFO_GOALS_REACHED_STEP 0
#define MAPF_INFO_GOALS_REACHED_TOTAL 1
#define MAPF_INFO_BLOCKING_COUNT_STEP 2
#define MAPF_INFO_BLOCKING_COUNT_TOTAL 3
#define MAPF_INFO_DEADLOCK_STEP 4
#define MAPF_INFO_LIVELOCK_STEP 5
#define MAPF_INFO_DEADLOCK_EVENT_STEP 6
#define MAPF_INFO_LIVELOCK_EVENT_STEP 7
#define MAPF_INFO_DEADLOCK_EVENTS_TOTAL 8
#define MAPF_INFO_LIVELOCK_EVENTS_TOTAL 9
#define MAPF_INFO_DEADLOCK_STEPS_TOTAL 10
#define MAPF_INFO_LIVELOCK_STEPS_TOTAL 11
#define MAPF_INFO_COMPLETION_RATIO 12 /* emitted by the reference only in lifelong mode; always computed here */
#define MAPF_INFO_THROUGHPUT 13       /* idem */

/* per-env counters of mapf_state.counters[B][MAPF_NUM_COUNTERS] */
#define MAPF_NUM_COUNTERS 16
#define MAPF_CTR_STEP_COUNT 0           /* step_count                         MA-env:37  */
#define MAPF_CTR_HIST_ROWS 1            /* rows appended to the lock history since its reset (unsaturated) */
#define MAPF_CTR_BLOCKING_COUNT 2       /* _episode_blocking_count            MA-env:63  */
#define MAPF_CTR_GOALS_REACHED_TOTAL 3  /* _episode_goals_reached_total       MA-env:88  */
#define MAPF_CTR_DEADLOCK_EVENTS 4      /* _episode_deadlock_events           MA-env:64  */
#define MAPF_CTR_LIVELOCK_EVENTS 5
#define MAPF_CTR_DEADLOCK_STEPS 6
#define MAPF_CTR_LIVELOCK_STEPS 7
#define MAPF_CTR_LOCK_STATE_PREV 8      /* bit0 _deadlock_state_prev, bit1 _livelock_state_prev MA-env:68-69 */
#define MAPF_CTR_EPISODES_DONE 9        /* episodes finished by this env since create (auto-reset bookkeeping) */
#define MAPF_CTR_MAY_FINISH 10          /* engine-internal hint, nonzero = the episode may end in the next step (step limit
                                         * reached, or every agent within one cell of its goal): the background sampler
                                         * leaves such envs alone.  Written by every step; every writer of positions, goals
                                         * or counters outside a step (mapf_set_state, mapf_reset, mapf_assign_new_goal)
                                         * must leave it non-zero.  mapf_get_state reports 0, mapf_debug_hints the word. */

/* per-env lifetime sums over finished episodes, mapf_get_episode_stats() adds them up over the envs:
 * the quantities the reference's RLlib callbacks log at episode end (src/trainers/callbacks.py:135-345).
 * A MAPF_FLAG_SINGLE_AGENT handle fills EPISODES, SUCCESSES, GOALS_REACHED and COMPLETED_AGENTS (both: agents with
 * goal_reached_once set, SA-env has no _episode_goals_reached_total), BLOCKING_COUNT (_episode_blocking_count, SA-env:317)
 * and EPISODE_STEPS; SA-env has no lock metrics, so its deadlock / livelock columns stay 0.  A step that latched an
 * invalid action books nothing (SA-env raises before the episode can end). */
#define MAPF_NUM_EPISODE_ACC 12
#define MAPF_ACC_EPISODES 0
#define MAPF_ACC_SUCCESSES 1        /* terminated and not truncated (SuccessRateCallback, finite mode) */
#define MAPF_ACC_GOALS_REACHED 2    /* sum of _episode_goals_reached_total at episode end */
#define MAPF_ACC_BLOCKING_COUNT 3
#define MAPF_ACC_DEADLOCK_COUNT 4   /* rising-edge events */
#define MAPF_ACC_LIVELOCK_COUNT 5
#define MAPF_ACC_DEADLOCK_STEPS 6
#define MAPF_ACC_LIVELOCK_STEPS 7
#define MAPF_ACC_COMPLETED_AGENTS 8 /* agents with _completed_once_arr set at episode end (completion_ratio numerator) */
#define MAPF_ACC_EPISODE_STEPS 9    /* sum of step_count at episode end */

typedef struct mapf_config {
    int32_t num_envs;           /* B >= 1 */
    int32_t height, width;      /* grid shape, each <= MAPF_MAX_DIM */
    int32_t num_agents;         /* N <= MAPF_MAX_AGENTS */
    int32_t sensor_range;       /* MA-env:40 */
    int32_t steps_per_episode;  /* MA-env:38 */
    uint32_t flags;             /* MAPF_FLAG_* */
    int32_t deadlock_window_steps; /* MA-env:56, clamped to >= 1 */
    int32_t livelock_window_steps; /* MA-env:57 */
    int32_t lock_nearby_manhattan; /* MA-env:58 */
    int32_t lock_min_neighbors;    /* MA-env:60 */
    double lock_progress_epsilon;  /* MA-env:59 */
    int32_t device;             /* HIP device ordinal */
    int32_t lanes_per_env;      /* 0 = auto (smallest power of two >= max(N,4)); else 4/8/16/32/64 */
} mapf_config;

typedef struct mapf_engine *mapf_handle;

/* host views for mapf_get_state / mapf_set_state; NULL members are skipped */
typedef struct mapf_state {
    int16_t *positions;      /* [B][N][2] (row, col)  _positions_arr */
    int16_t *goals;          /* [B][N][2]             _goals_arr */
    int16_t *starts;         /* [B][N][2]             _starts_arr */
    uint8_t *reached;        /* [B][N]                _reached_arr (sticky) */
    uint8_t *completed_once; /* [B][N]                _completed_once_arr */
    uint8_t *pressure_prev;  /* [B][N]  0/1           _blocking_pressure_prev_arr */
    int32_t *counters;       /* [B][MAPF_NUM_COUNTERS] */
    uint64_t *rng_words;     /* [B][6] numpy PCG64: state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger */
    uint64_t *lock_history;  /* [B][N][3] shift registers, bit k = flag k steps ago: moved, failed_move, goal_progress.
                              * A handle with max(deadlock_window_steps, livelock_window_steps) <= 16 keeps 16 bits of each
                              * (mapf_state_bytes_per_agent == 32, or 16): mapf_get_state reports bits 16..63 as zero and
                              * mapf_set_state ignores them.  No output of a step depends on them -- every use of a register is
                              * masked by a window -- and get_state -> set_state -> get_state is the identity either way. */
    int16_t *distance_ring;  /* [B][livelock_window][N], slot = history row index mod livelock_window */
} mapf_state;

uint32_t mapf_version(void);
/* flat observation length L for a config (MA-env:214-236): V*V + 2 [+1] [+1] [+5] */
int32_t mapf_obs_len(const mapf_config *cfg);

/* mapf_create also picks the build of the step kernel by the size of its grid: small-group configurations (at most 16
 * lanes per env) exist for two register budgets, and a grid of more than three waves per SIMD gets the 128-register
 * one.  MAPF_FLAG_FORCE_DENSE / MAPF_FLAG_FORCE_SPARSE override the choice (test knobs; results are
 * identical either way).  The library reads no environment variable except MAPF_JIT_CACHE_DIR (and XDG_CACHE_HOME /
 * HOME behind it) for the on-disk cache of MAPF_FLAG_JIT_SPECIALIZE. */
int mapf_create(const mapf_config *cfg /* host */, mapf_handle *out);
int mapf_destroy(mapf_handle h);
const char *mapf_last_error(mapf_handle h); /* h may be NULL: error of the last failed mapf_create */

/* grids: host uint8 [B][H][W] (shared == 0) or one [H][W] used by every env (shared != 0); 0 free, 1 obstacle.
 * Fails with MAPF_ERR_FEW_FREE when an env has fewer than 2N free cells (reference ctor, MA-env:270-275). */
int mapf_set_grids(mapf_handle h, const uint8_t *grids /* host */, int32_t shared);

/* numpy Generator(PCG64) state per env, host uint64 [B][6] (see mapf_state.rng_words).  Seed expansion
 * (SeedSequence) is the caller's job: np.random.default_rng(seed).bit_generator.state (MA-env:74-78). */
int mapf_set_rng_state(mapf_handle h, const uint64_t *rng_words /* host */);

/* deterministic mode (MA-env:124-132): fixed starts / goals, host int16 [B][N][2] each; also places agents. */
int mapf_set_fixed_starts_goals(mapf_handle h, const int16_t *starts /* host */, const int16_t *goals /* host */);

int mapf_get_state(mapf_handle h, mapf_state *out /* host views */);
int mapf_set_state(mapf_handle h, const mapf_state *in /* host views */);

/* reset (MA-env:440-472).  env_mask: device uint8 [B], nonzero = reset that env; NULL = all.
 * obs: device float32 [B][N][L], rows of reset envs are written, rows of all other envs are left alone; may be NULL
 * (state only -- the reference ctor's own generate_starts_goals() draw, MA-env:133-134, is mapf_reset with obs NULL). */
int mapf_reset(mapf_handle h, const uint8_t *env_mask /* device */, float *obs /* device */, void *stream);

/* one step of every env (MA-env:474-695).  All pointers device; any output may be NULL.
 *   actions     int8   [B][N]      0 NO_OP, 1 UP, 2 RIGHT, 3 DOWN, 4 LEFT (actions.py:1-5)
 *   obs         float32[B][N][L]   per-agent flat observation, reference layout (MA-env:306-328)
 *   rewards     float32[B][N]
 *   terminated  uint8  [B]         terminated["__all__"]   (per-agent flags equal it, MA-env:668-690)
 *   truncated   uint8  [B]         truncated["__all__"]
 *   info_all    float32[B][14]     MAPF_INFO_* columns
 *   info_agent  uint8  [B][N][2]   {blocking, goal_reached_step}  (MA-env:627-629)
 *   final_obs   float32[B][N][L]   only with auto_reset: terminal observation of envs that finished
 * auto_reset != 0: an env whose episode ended is reset() inside the same launch, exactly as the reference
 * harness does right after the step (scripts/benchmark_multi_agent_env.py:89-95); its `obs` rows then hold
 * the reset observation.
 * What is written: obs, rewards, terminated, truncated, info_all and info_agent, each that is not NULL, for EVERY env,
 * whichever others are NULL.  final_obs: with auto_reset != 0 the rows of the envs that finished in this step, and those
 * alone -- rows of an env that did not finish are left alone (every kernel family; they are NOT a copy of obs).  With
 * auto_reset == 0 final_obs is ignored: it may be passed, and is left alone entirely (the terminal observation then is in
 * obs).
 * An env that latched an invalid action (MAPF_ERR_BAD_ACTION; the reference raises inside step() and returns nothing):
 * its rows of EVERY output of that step, final_obs included, are left alone, in every kernel family and in the fused
 * launches (there: its rows of that step's slab); the rows of all other envs are written as usual.  A caller that cannot
 * poll before it reads the outputs should clear them first (the batched wrappers zero-fill what they hand to
 * mapf_cte_step_many for this reason). */
int mapf_step(mapf_handle h, const int8_t *actions, float *obs, float *rewards, uint8_t *terminated, uint8_t *truncated,
              float *info_all, uint8_t *info_agent, float *final_obs, int32_t auto_reset, void *stream);

/* mapf_step for a SUBSET of the envs: env_mask (device uint8 [B]) selects the envs that step; every other env is not
 * touched at all -- state, generator, counters, episode statistics, error latch -- and its rows of the outputs are
 * left as they are.  This is what stepping ONE of several reference env objects means (RLlib's runners step their
 * sub-envs one by one, and skip the ones that wait for a reset: MultiAgentEnv.step per object, MA-env:474); the vector
 * adapters use it for rows stepped alone and for the next-step autoreset of the new-stack vector protocol. */
int mapf_step_masked(mapf_handle h, const int8_t *actions, const uint8_t *env_mask, float *obs, float *rewards,
                     uint8_t *terminated, uint8_t *truncated, float *info_all, uint8_t *info_agent, float *final_obs,
                     int32_t auto_reset, void *stream);

/* T consecutive steps in ONE launch (state stays in registers, obstacle rows in LDS): what the reference's
 * env-only benchmark loop does when the actions do not depend on the observations
 * (scripts/benchmark_multi_agent_env.py:85-95, mode "random"), or any scripted / pre-sampled action stream.
 *   actions  device int8 [T][B][N]
 *   obs      device float32; obs_mode 0: unused -- may be NULL, and a pointer that is passed is left alone, not one byte
 *            of it is written; 1: [B][N][L] observation after the last step, exactly one slab; 2: [T][B][N][L] every step
 *   rewards [T][B][N], terminated / truncated [T][B], info_all [T][B][14], info_agent [T][B][N][2]; any may be NULL
 * Finished envs are reset inside the loop (auto_reset semantics of mapf_step: the observation of a step that
 * ended an episode is the reset observation). */
int mapf_step_many(mapf_handle h, int32_t T, const int8_t *actions, float *obs, int32_t obs_mode, float *rewards,
                   uint8_t *terminated, uint8_t *truncated, float *info_all, uint8_t *info_agent, void *stream);

/* The same fused launch with a DEVICE-SIDE action source, for loops whose actions depend on the observations: the
 * masked-random policy of the reference's benchmark (scripts/benchmark_multi_agent_env.py:42-57, mode "masked": every
 * agent picks uniformly among the actions its action mask allows) evaluated in-kernel, step after step, on the
 * observation the previous step produced -- obs_in [B][N][L] (device) for the first step.  The generator is
 * counter-based (a hash of seed, env, agent and step index), so a run is reproducible and has no state; it is NOT
 * NumPy's stream: the actions taken are returned in actions_out [T][B][N] (device) and replaying them through
 * mapf_step / mapf_step_many gives the same transitions.  Needs MAPF_FLAG_ACTION_MASK; obs [T][B][N][L] is written for
 * every step (it is what the policy reads); the other outputs are as in mapf_step_many. */
int mapf_step_many_sampled(mapf_handle h, int32_t T, const float *obs_in, uint64_t seed, int8_t *actions_out, float *obs,
                           float *rewards, uint8_t *terminated, uint8_t *truncated, float *info_all, uint8_t *info_agent,
                           void *stream);

/* ---- single-agent (CTE) sibling env: reference src/environments/reference_model_single_agent.py ("SA-env") ----
 * One policy drives all N agents (gym.Env, MultiDiscrete([5]*N) action).  Create the handle with
 * MAPF_FLAG_SINGLE_AGENT (only MAPF_FLAG_DETERMINISTIC is meaningful besides it; sensor_range and the lock
 * settings are unused), then set grids / RNG / fixed tables as usual.  Flat observation = H*W cell codes
 * (0 free, 1 obstacle, 2+2i agent i, 3+2i goal i; SA-env:407-441) followed by the joint 5N action mask
 * (SA-env:443-495); mapf_obs_len() returns H*W + 5N.
 *   mapf_cte_configure  <- blocking_penalty / move_after_goal_penalty of the ctor   SA-env:92-93 (defaults -0.2, -0.05)
 *   mapf_cte_reset      <- reset()   SA-env:222-244 (+ generate_starts_goals :158-191); obs NULL = the ctor's draw :113-114
 *   mapf_cte_step       <- step()    SA-env:246-363:  reward double [B] (the reference's float64 sum, same order of
 *                          additions), terminated / truncated uint8 [B], info float32 [B][4] =
 *                          {blocking_count_step, goals_reached_step, goals_reached_total, blocking_count_total};
 *                          info["action_mask"] is the tail of the observation.
 *   mapf_cte_step_masked <- step() of SOME of the envs (below)
 *   mapf_get_episode_stats / mapf_episode_stats_async <- what the callbacks read at episode end (MAPF_ACC_* above) */
int mapf_cte_configure(mapf_handle h, double blocking_penalty, double move_after_goal_penalty);
int mapf_cte_reset(mapf_handle h, const uint8_t *env_mask /* device */, float *obs /* device */, void *stream);
int mapf_cte_step(mapf_handle h, const int8_t *actions, float *obs, double *reward, uint8_t *terminated,
                  uint8_t *truncated, float *info, float *final_obs, int32_t auto_reset, void *stream);

/* mapf_cte_step for a SUBSET of the envs (the contract of mapf_step_masked): env_mask (device uint8 [B]) selects the envs
 * that step; every other env is not touched at all -- state and visible stream (mapf_get_state), counters and hint,
 * episode statistics, error latch -- and its rows of every output, the obstacle floats of its observation row included,
 * are left as they are.  Replaces SA-env:246-363 called on SOME of a runner's env objects: RLlib's new-stack single-agent
 * runner steps its sub-envs as one vector env with next-step autoreset (src/agents/ppo.py:24-44), where the rows that
 * finished in the previous call wait for their reset (mapf_cte_reset with the complementary mask) while the others step.
 * A masked launch pre-draws no next-episode placement; a stepped env that ends its episode without one draws inline.
 * final_obs, the rows of an env that latched an invalid action and obs with obs_mode 0 follow the rules stated at mapf_step /
 * mapf_step_many: final_obs rows of envs that did not finish (and all of it with auto_reset == 0) are left alone, the
 * failed env's rows of every output are left alone, an obs pointer passed with obs_mode 0 is left alone. */
int mapf_cte_step_masked(mapf_handle h, const int8_t *actions, const uint8_t *env_mask, float *obs, double *reward,
                         uint8_t *terminated, uint8_t *truncated, float *info, float *final_obs, int32_t auto_reset,
                         void *stream);

/* T consecutive steps of the single-agent env in ONE launch for an action stream known up front (the CTE counterpart of
 * mapf_step_many; the reference's loop is `for t: obs, r, term, trunc, info = env.step(a[t]); if term or trunc:
 * env.reset()` around SA-env:246-363 / :222-244): positions stay in registers, the obstacle part of the full-grid
 * observation row is written once per launch, per step only the actions are read and the outputs written.
 *   actions device int8 [T][B][N];  obs_mode 0: no observation, 1: [B][H*W+5N] after the last step, 2: [T][B][H*W+5N];
 *   reward [T][B] float64, terminated / truncated [T][B], info [T][B][4]; any may be NULL.
 * Finished envs are reset inside the loop; the observation of a step that ended an episode is the reset observation. */
int mapf_cte_step_many(mapf_handle h, int32_t T, const int8_t *actions, float *obs, int32_t obs_mode, double *reward,
                       uint8_t *terminated, uint8_t *truncated, float *info, void *stream);

/* The same step for callers that pay per ARGUMENT (ctypes from a Python rollout loop: ~0.4 us each): the output buffers of
 * mapf_step are bound to the handle once, mapf_step_bound(h, actions, auto_reset, stream) then is mapf_step with those
 * pointers and final_obs = NULL.  The buffers stay the caller's; binding again replaces them. */
int mapf_bind_outputs(mapf_handle h, float *obs, float *rewards, uint8_t *terminated, uint8_t *truncated, float *info_all,
                      uint8_t *info_agent);
int mapf_step_bound(mapf_handle h, const int8_t *actions, int32_t auto_reset, void *stream);

/* observation of every agent from the CURRENT state, nothing is modified: what the reference returns when
 * get_obs / get_action_mask / _flatten_observation (MA-env:707-773, :306-328) are called outside step().
 * obs: device float32 [B][N][L]. */
int mapf_observe(mapf_handle h, float *obs /* device */, void *stream);

/* one goal respawn of one agent OUTSIDE step(): `_assign_new_goal(agent_idx)` (MA-env:284-304) -- clears the agent's goal,
 * counts the k free cells (row-major `_free_positions`) that hold no agent and no goal, draws rng.integers(k) from the
 * env's stream (nothing is drawn when k == 1), stores the r-th such cell as the new goal and returns it in
 * new_goal (host int16 [2]: row, col).  Runs on `stream` and waits for it.  MAPF_ERR_NO_RESPAWN when k == 0 (the
 * reference's RuntimeError, :296-298; also latched for mapf_poll_error).  Inside mapf_step the respawns of lifelong
 * mode run in the step kernel; this entry point is the helper by itself, as the reference's tests call it. */
int mapf_assign_new_goal(mapf_handle h, int32_t env, int32_t agent, int16_t *new_goal /* host */, void *stream);

/* sums of the per-env episode accumulators over all envs of the handle (either variant: see MAPF_ACC_* for the columns a
 * single-agent handle fills): host int64 out[MAPF_NUM_EPISODE_ACC];
 * reset != 0 clears them afterwards.  Synchronizes the device.  (Off the hot path; for a multi-GPU job add the
 * vectors of the ranks, e.g. one RCCL all-reduce of this 96-byte buffer per reporting interval.) */
int mapf_get_episode_stats(mapf_handle h, int64_t *out /* host */, int32_t reset);

/* the same sums without a host round trip: one small launch on `stream` adds the accumulators up into DEVICE memory
 * (int64 out[MAPF_NUM_EPISODE_ACC]); nothing is synchronized and nothing is cleared.  For a training loop that logs the
 * callbacks' metrics (src/trainers/callbacks.py:236-345) from a tensor every so often, and for bench.py, which must not
 * leave the GPU idle between its warm-up launches and the timed region. */
int mapf_episode_stats_async(mapf_handle h, int64_t *out /* device */, void *stream);

/* read (and clear) the device error record; synchronizes `stream`.  Returns MAPF_OK when no env has
 * failed, else the code of the first failure with its env / agent / offending value. */
int mapf_poll_error(mapf_handle h, void *stream, int32_t *env, int32_t *agent, int32_t *value);

/* diagnostic builds only (-DMAPF_STAMPS; the shipped library returns MAPF_ERR_STATE): copies the per-wave
 * s_memtime stamps of the last mapf_step to host uint64 out[workgroups][32]; returns the number of words. */
int mapf_debug_stamps(mapf_handle h, uint64_t *out /* host */, int32_t max_words);

/* diagnostic: the placement slots [B][N] (mapf_kernels.inl: kSlotInvalid / kSlotStaged*), the staging buffer of the
 * background draw [B][4N+4] and the visible stream states [B][6] as they are on the device (host outputs, any may be
 * NULL).  Synchronizes the device. */
int mapf_debug_slots(mapf_handle h, uint32_t *slots /* host */, uint32_t *stage /* host */, uint64_t *vis /* host */);

/* diagnostic: word MAPF_CTR_MAY_FINISH of every env as it is on the device (mapf_get_state zeroes it).  Synchronizes the
 * device. */
int mapf_debug_hints(mapf_handle h, int32_t *out /* host, [B] */);

/* 1 = this handle steps with a kernel compiled for its configuration at mapf_create (MAPF_FLAG_JIT_SPECIALIZE), 0 = not;
 * *why (may be NULL) gets a static or handle-owned string: the reason when 0, the compile time when 1. */
int mapf_jit_status(mapf_handle h, const char **why);

/* dynamic-LDS bytes and grid size the step kernel is launched with (for DESIGN.md / profiling notes).
 * Returns >= 0: the id of the compile-time specialisation of the step kernel in use (0 = runtime-config kernel). */
int mapf_launch_info(mapf_handle h, int32_t *blocks, int32_t *threads, int32_t *lds_bytes, int32_t *lanes_per_env);
/* bytes of agent state the handle keeps per agent on the device: 48 with a lock window above 16 steps; 32 when both are
 * <= 16 steps (16-bit lock history, see mapf_state.lock_history); 16 when, in addition, episodes are finite (no
 * MAPF_FLAG_LIFELONG) and the config asks for it (MAPF_FLAG_DERIVED_DISTANCE): the goal then stays put for an episode, a move changes the distance to it by exactly one, and the
 * handle keeps one bit per step ("the distance went down") instead of the 16 distance bytes.  mapf_get_state rebuilds the
 * numeric distance_ring from the bits, mapf_set_state turns a ring into bits.  A state the bits cannot express -- a ring
 * that is no one-cell walk of the moved bits, positions or goals set under an existing history, mapf_assign_new_goal on
 * such a handle -- converts the handle, once and for good, to the 32-byte layout (the distances the caller supplied are
 * kept as numbers; a prebuilt specialisation carries kernels for both layouts, a handle compiled with
 * MAPF_FLAG_JIT_SPECIALIZE goes on with the runtime-config kernels; graphs captured before must be captured again): the value returned
 * here changes from 16 to 32.  A negative error code for a NULL handle. */
int mapf_state_bytes_per_agent(mapf_handle h);
/* The two conversions behind that, for ONE env, pure host functions (no device, no handle): ring [lw][N] int16 (slot =
 * history row index mod lw), hist_rows = the env's MAPF_CTR_HIST_ROWS, positions / goals [N][2], lock_history [N][3]
 * (only the moved register is read), down [N] (bit k = the step k rows back brought the agent one cell closer).
 * mapf_derived_to_ring writes the min(hist_rows, lw) rows that exist and zero elsewhere.  mapf_derived_from_ring returns 1
 * when the bits express the ring, 0 when they cannot. */
void mapf_derived_to_ring(const uint16_t *down, int32_t lw, int32_t n_agents, int32_t hist_rows, const int16_t *positions,
                          const int16_t *goals, const uint64_t *lock_history, int16_t *ring);
int mapf_derived_from_ring(const int16_t *ring, int32_t lw, int32_t n_agents, int32_t hist_rows, const int16_t *positions,
                           const int16_t *goals, const uint64_t *lock_history, uint16_t *down);
/* the same for the fused launches of a MAPF_FLAG_SINGLE_AGENT handle (mapf_cte_step_many with T > 1), which pick their
 * own group width; MAPF_ERR_STATE for other handles. */
int mapf_cte_many_launch_info(mapf_handle h, int32_t *blocks, int32_t *threads, int32_t *lds_bytes, int32_t *lanes_per_env);

/* rgb_array frames of K envs of the handle (either kind), from the state the handle holds (what mapf_get_state reports:
 * with in-kernel auto-reset that is the new episode's placement).  The reference draws with matplotlib patches
 * (MA-env:775-916); this is an exact integer raster of the grid area with the same layers, colours and draw order and no
 * axes, margins or anti-aliasing, so a restatement in NumPy reproduces it bit for bit.
 *   frames   device uint8 [K][H*c][W*c][3] RGB, c = cell_px in [MAPF_RENDER_MIN_CELL_PX, MAPF_RENDER_MAX_CELL_PX];
 *            pixel row 0 is grid row 0 (the reference's inverted y axis), pixel (y, x) lies in cell (i, j) = (y / c, x / c)
 *   env_ids  device int32 [K]: frame k shows env env_ids[k] (any order, duplicates allowed); NULL = envs 0 .. K-1
 *            (then K <= B).  An id outside [0, B) gives an all-zero frame and latches MAPF_ERR_CONFIG (env = k, value = the
 *            id) in the device error record (mapf_poll_error), like a bad action.
 * The rule, all integer arithmetic.  For pixel (y, x) in cell (i, j), its offsets from the cell centre in half pixels are
 * dx = 2x + 1 - c(2j + 1), dy = 2y + 1 - c(2i + 1); blend(d, s, a) = (s*a + d*(255 - a) + 127) / 255 per channel.
 *   1. base: black (0,0,0) on an obstacle cell, else white (255,255,255)
 *   2. grid line: y % c == 0 or x % c == 0 -> gray (128,128,128), obstacle cells included
 *   3. goal: (i, j) is the goal of agent g and |dx| + |dy| <= c -> blend(colour, PALETTE[g % 16], 128)
 *   4. for a = 0 .. N-1 in order:
 *        disc:   agent a stands on (i, j) and 25(dx^2 + dy^2) <= 9c^2 (radius 0.3 cell) -> PALETTE[a % 16], opaque
 *        window: multi-agent handles only (SA-env draws none): |i - row_a| <= sensor_range and |j - col_a| <= sensor_range
 *                -> blend(colour, PALETTE[a % 16], 51)
 * PALETTE, the reference's 16 colours in order: FF0000 red, 0000FF blue, 008000 green, 800080 purple, FFA500 orange,
 * 00FFFF cyan, FF00FF magenta, FFFF00 yellow, A52A2A brown, FFC0CB pink, 808000 olive, 008080 teal, 000080 navy,
 * FFD700 gold, 00FF00 lime, 808080 gray.
 * Asynchronous on `stream`: one launch, no allocation, no synchronisation (graph-capturable).  Reads the agent positions,
 * goals and obstacle rows only; writes the frames (and the error record for a bad id), nothing else.
 * MAPF_ERR_CONFIG: null handle or frames, K < 1, cell_px out of range, env_ids NULL with K > B.  MAPF_ERR_STATE: before
 * mapf_set_grids. */
int mapf_render(mapf_handle h, const int32_t *env_ids /* device [K] or NULL */, int32_t K, int32_t cell_px,
                uint8_t *frames /* device [K][H*c][W*c][3] */, void *stream);

/* Batched evaluation: the bookkeeping of the reference's test mode (main.py test_trained_model) on the device, for every env
 * of a multi-agent handle at once.  The reference runs `num_episodes` times reset() + step() until done, and keeps one result
 * row per episode (main.py:286-324) and one visit count per cell, incremented after every step on the cell of every agent
 * (main.py:153-155, :262-267).  Here every env runs episodes_per_env = E episodes of its own; one step of the evaluation is
 * three launches on one stream and nothing else:
 *     mapf_step_masked(h, actions, active, ..., auto_reset = 0)     envs that have finished their E episodes idle, untouched
 *     mapf_eval_record(h, rewards, terminated, truncated, info_all)
 *     mapf_reset(h, reset_mask, obs)                                the reference's env.reset() of main.py:174
 * All buffers are device memory owned by the caller:
 *   heat              uint32 [B][H][W]      visits: +1 on the cell of every agent after every step of an active env, the
 *                                           terminal step included, the placement of the following reset not included
 *   ep_i32            int32  [B][E][2 + 4N] episode k of env b: timesteps, flags (bit 0 terminated, bit 1 truncated), then per
 *                                           agent start row, start col, goal row, goal col -- the goals as they are when the
 *                                           episode ends (what env.goals holds at main.py:315; lifelong mode: the last goal)
 *   ep_f64            double [B][E][1 + N]  total reward (main.py:237), then the reward of every agent (main.py:263); rewards
 *                                           are multiples of 0.5, so these sums are exact whatever the order of addition
 *   ep_info           float  [B][E][14]     the terminal step's info_all row as it is (MAPF_INFO_* columns)
 *   episodes_recorded int32  [B]            episodes of env b recorded so far: slots k < episodes_recorded[b] are valid
 *   active            uint8  [B]            the env mask of mapf_step_masked: 1 while the env has episodes left to run
 *   reset_mask        uint8  [B]            the env mask of mapf_reset: 1 where the step just recorded ended an episode and
 *                                           the env runs another one; 0 elsewhere, and for good once an env has finished
 * mapf_eval_begin binds the buffers to the handle, zeroes heat, episodes_recorded, reset_mask and the handle's running sums
 * (float64 [B][N] and int32 [B], allocated here, freed by mapf_eval_end or mapf_destroy) and sets active to 1, all enqueued
 * on `stream`; the episode records need no clearing.  It does not reset the envs: the caller's mapf_reset(h, NULL, obs)
 * starts the first episodes.
 * mapf_eval_record books the step just made, for envs with active[b] != 0 only (nothing of another env is read or
 * written): adds the rewards to the running sums, counts the step and the visits, and where terminated | truncated is set
 * writes record k = episodes_recorded[b], clears the env's running sums, increments episodes_recorded[b] and sets
 * reset_mask[b] = 1 -- unless that was the env's E-th episode: then it clears active[b] and writes reset_mask[b] = 0, and the
 * env keeps its terminal state from then on.  Otherwise reset_mask[b] = 0.  The pointers are those of the step's outputs
 * (device).  One launch, asynchronous on `stream`, no allocation, no synchronisation (graph-capturable); it reads plane 0 of
 * the agent state and changes nothing the step kernels read: mapf_get_state before and after it is identical.
 * MAPF_ERR_CONFIG: null handle or buffer, episodes_per_env < 1.  MAPF_ERR_STATE: mapf_eval_record without mapf_eval_begin,
 * before mapf_set_grids, or either call on a MAPF_FLAG_SINGLE_AGENT handle (the reference's test mode is multi-agent only,
 * "test only works with CTDE for now", main.py:37; the single-agent env has its own pair of calls, mapf_cte_eval_begin /
 * mapf_cte_eval_record below).  mapf_eval_end waits for the device and unbinds; it serves handles of either kind. */
int mapf_eval_begin(mapf_handle h, int32_t episodes_per_env, uint32_t *heat, int32_t *ep_i32, double *ep_f64,
                    float *ep_info, int32_t *episodes_recorded, uint8_t *active, uint8_t *reset_mask, void *stream);
int mapf_eval_record(mapf_handle h, const float *rewards, const uint8_t *terminated, const uint8_t *truncated,
                     const float *info_all, void *stream);
int mapf_eval_end(mapf_handle h);

/* The same bookkeeping for a MAPF_FLAG_SINGLE_AGENT handle: main.py's test loop (main.py:172-324) restated for a gym.Env --
 * reset(), step() until `terminated or truncated`, `episode_reward += reward`, after every step one visit on the cell of every
 * agent (the terminal step included, the placement of the next reset not included), one record per episode.  One step of the
 * evaluation is three launches on one stream and nothing else:
 *     mapf_cte_step_masked(h, actions, active, ..., auto_reset = 0)
 *     mapf_cte_eval_record(h, reward, terminated, truncated, info)
 *     mapf_cte_reset(h, reset_mask, obs)
 * The buffers are the caller's device memory, as above, with the single-agent env's layout:
 *   heat              uint32 [B][H][W]
 *   ep_i32            int32  [B][E][2 + 4N] timesteps, flags, then per agent start row, start col, goal row, goal col as the
 *                                           handle holds them when the episode ends.  Flag bit 0 is terminated, bit 1
 *                                           truncated; an episode that ends at the time limit sets BOTH (SA-env:347-348), so
 *                                           success is bit 0 without bit 1
 *   ep_f64            double [B][E]         the episode's total reward.  The step rewards carry -0.2 and -0.05 terms, so this
 *                                           sum is NOT free of the order of addition: it is a running float64 sum per env,
 *                                           run = run + reward[b] once per step in step order and cleared when the episode is
 *                                           recorded -- Python's `episode_reward += reward`, bit for bit
 *   ep_info           float  [B][E][4]      the terminal step's info row as it is (mapf_cte_step's columns)
 *   episodes_recorded, active, reset_mask   as stated at mapf_eval_begin
 * mapf_cte_eval_begin binds the buffers, zeroes heat, episodes_recorded, reset_mask and the handle's running sums (float64 [B]
 * and int32 [B], allocated here, freed by mapf_eval_end or mapf_destroy) and sets active to 1, all enqueued on `stream`.  It
 * does not reset the envs.
 * mapf_cte_eval_record: one launch, asynchronous on `stream`, no allocation, no synchronisation, no atomics (graph-capturable
 * from the first call).  It touches only envs with active[b] != 0, reads plane 0 of the agent state and changes nothing the
 * step kernels read (mapf_get_state before and after it is identical), and writes record slot k = episodes_recorded[b] only
 * for an env whose episode just ended.
 * MAPF_ERR_CONFIG: null handle or buffer, episodes_per_env < 1.  MAPF_ERR_STATE: either call on a multi-agent handle,
 * mapf_cte_eval_record without mapf_cte_eval_begin, after mapf_eval_end or before mapf_set_grids.  Nothing is launched on
 * any of them. */
int mapf_cte_eval_begin(mapf_handle h, int32_t episodes_per_env, uint32_t *heat, int32_t *ep_i32, double *ep_f64,
                        float *ep_info, int32_t *episodes_recorded, uint8_t *active, uint8_t *reset_mask, void *stream);
int mapf_cte_eval_record(mapf_handle h, const double *reward, const uint8_t *terminated, const uint8_t *truncated,
                         const float *info, void *stream);

/* Evaluation trace: the per-step state of K chosen envs of an evaluation, kept on the device so that every frame of their
 * episodes can be redrawn afterwards (mapf_render_words) and every agent's path read back -- what main.py's test mode
 * shows as a video (SAVE_VIDEO, main.py:49-53, :188-194, :239-243, :269-274, :342-347) and what scripts/a-star.py and
 * scripts/cbs.py print and measure per agent.  Handles of either kind.  The calls need a bound evaluation (mapf_eval_begin /
 * mapf_cte_eval_begin) and are unbound by mapf_eval_end, or by the next *_eval_begin.
 *   words    device uint32 [K][V][S + 1][N], S = the handle's steps_per_episode, V = `episodes`: slot (k, v, t) holds the
 *            state of env env_ids[k] after step t of its episode v; t = 0 is the placement the episode started from.  A WORD
 *            (part of this ABI) is the agent's plane-0 word as the rasteriser reads it:
 *                col | row << 8 | goal_col << 16 | goal_row << 24
 *            Every episode ends at the step limit at the latest, so a slot is a fixed address: no cursor, no atomic.  The
 *            length of episode (k, v) is the `timesteps` the recorder writes into ep_i32; slots with t above it, and the
 *            slots of episodes the env did not run, are never written.  The caller owns the buffer; nothing clears it.
 *   env_ids  device int32 [K]: any order, duplicates allowed (each k has its own region).  An id outside [0, B) writes
 *            nothing and latches MAPF_ERR_CONFIG (env = k, value = the id) in the device error record, as in mapf_render.
 * mapf_eval_trace(h, phase): with b = env_ids[k] and v = episodes_recorded[b], nothing is written unless v < V, and
 *   MAPF_TRACE_START  words[k][0][0][:] takes the words of env b.  Call it once, after the evaluation's first mapf_reset /
 *                     mapf_cte_reset.
 *   MAPF_TRACE_STEP   if active[b]: words[k][v][t][:] is written, t = the steps of the running episode with the step just
 *                     made (the recorder's running count + 1), the terminal step included; in lifelong mode the goals are
 *                     the ones the step left.  Call it after the masked step and BEFORE mapf_eval_record /
 *                     mapf_cte_eval_record: the recorder moves v and t on to the next episode.
 *   MAPF_TRACE_RESET  if reset_mask[b]: words[k][v][0][:] is written (v already counts the finished episode).  Call it
 *                     after the masked reset.
 * so a traced step of an evaluation is five launches: masked step, trace STEP, recorder, masked reset, trace RESET.
 * mapf_eval_trace is exactly one launch, asynchronous on `stream`, its grid sized by K (not by B); no allocation, no
 * workspace, no synchronisation, graph-capturable from its first call.  It reads plane 0 of the agent state and the
 * recorder's active, reset_mask, episodes_recorded and running step count, and writes nothing but `words`:
 * mapf_get_state and every recorder buffer are identical before and after it.  mapf_eval_trace_begin enqueues nothing.
 * MAPF_ERR_CONFIG, and nothing is launched: a null argument, K < 1, episodes < 1, an unknown phase.  MAPF_ERR_STATE, and
 * nothing is launched: no bound evaluation, mapf_eval_trace without mapf_eval_trace_begin or before mapf_set_grids.  The
 * checking build (-DMAPF_CHECK) range-checks the slot index (site 26). */
#define MAPF_TRACE_START 0 /* after the evaluation's first mapf_reset / mapf_cte_reset: frame 0 of episode 0 */
#define MAPF_TRACE_STEP 1  /* after the masked step, BEFORE mapf_eval_record / mapf_cte_eval_record */
#define MAPF_TRACE_RESET 2 /* after the masked reset: frame 0 of the episode that just started */
int mapf_eval_trace_begin(mapf_handle h, int32_t K, const int32_t *env_ids /* device [K] */, int32_t episodes /* V */,
                          uint32_t *words /* device [K][V][S + 1][N] */, void *stream);
int mapf_eval_trace(mapf_handle h, int32_t phase, void *stream);

/* Frames from recorded words: the rule of mapf_render, word for word, with frame f drawn from words[rows[f]][:] (words as
 * stated at mapf_eval_trace_begin) instead of the state the handle holds, over the obstacle rows of env env_ids[f].  Sensor
 * windows are drawn on multi-agent handles only.
 *   words    device uint32 [M][N]: any M rows of N words, e.g. a trace viewed as [K * V * (S + 1)][N]
 *   rows     device int32 [F]: the row of `words` behind frame f, each in [0, M) (the caller's to keep: M is not passed); a
 *            row may repeat -- that is how a held last frame is drawn.  NULL = rows 0 .. F-1.  A negative row gives an all-
 *            zero frame and latches MAPF_ERR_CONFIG (env = f, value = the row).
 *   env_ids  device int32 [F]: whose obstacle rows (and sensor range) frame f is drawn over.  An id outside [0, B) gives an
 *            all-zero frame and latches MAPF_ERR_CONFIG (env = f, value = the id), as in mapf_render.
 *   frames   device uint8 [F][H*c][W*c][3], c = cell_px, as in mapf_render (any alignment)
 * An agent whose word lies outside the grid draws no disc and no diamond; whatever the words hold, nothing outside `frames`
 * is written.  One launch, asynchronous on `stream`, no allocation, no synchronisation (graph-capturable); reads `words`,
 * `rows`, `env_ids` and the obstacle rows, writes the frames (and the error record).  The kernel is the second
 * instantiation of mapf_render's, which differs in where the agent words are loaded from and in nothing else.
 * MAPF_ERR_CONFIG: null handle, words, env_ids or frames, F < 1, cell_px out of range.  MAPF_ERR_STATE: before
 * mapf_set_grids. */
int mapf_render_words(mapf_handle h, const uint32_t *words /* device [M][N] */, const int32_t *rows /* device [F] or NULL: 0 .. F-1 */,
                      const int32_t *env_ids /* device [F]: whose obstacle rows */, int32_t F, int32_t cell_px,
                      uint8_t *frames /* device [F][H*c][W*c][3] */, void *stream);

/* Shortest-path planner: breadth-first searches on the envs' own grids, on the device (handles of either kind).
 * The graph: nodes are the cells of an env's grid that are not obstacles, edges join the four neighbours; agents are never
 * obstacles for a distance.  d(env, x -> g) is the number of moves of a shortest path, -1 when there is none or when x or g
 * is an obstacle or lies outside the grid.  Action ids are the reference's (MA-env:104-113): 1 UP (row - 1), 2 RIGHT
 * (col + 1), 3 DOWN (row + 1), 4 LEFT (col - 1), 0 NO_OP.
 * The expert action of an agent on p with goal g and D = d(p -> g), positions and goals being what mapf_get_state reports
 * (what the next mapf_step starts from):
 *   D <= 0 (on its goal, or the goal is unreachable): 0
 *   mode 0, independent: the lowest action id whose target cell is inside the grid, is no obstacle and has
 *                        d(target -> g) = D - 1
 *   mode 1, yielding:    the same candidates without the target cells another agent of the env stands on; none left: 0
 * All three calls are pure functions of grids, positions and goals: asynchronous on `stream`, exactly one launch, no
 * allocation, no synchronisation (graph-capturable), no generator, and they change nothing the step kernels read:
 * mapf_get_state before and after is identical.  MAPF_ERR_CONFIG: null handle or buffer (dist may be NULL), a mode other than
 * 0 / 1, K < 1 -- nothing is launched.  MAPF_ERR_STATE: before mapf_set_grids.
 * An env id outside [0, B) latches MAPF_ERR_CONFIG (env = k, value = the id) in the device error record (mapf_poll_error),
 * like mapf_render, and row k of the output is not written. */

/* expert action of every agent (rule above).  Writes actions [B][N] int8 and, when not NULL, dist [B][N] int32 (D of the
 * agent) for every env and agent; nothing else. */
int mapf_expert_actions(mapf_handle h, int32_t mode, int8_t *actions /* device */, int32_t *dist /* device or NULL */,
                        void *stream);

/* Shortest-path guidance: what the expert decides from, as MAPF_GUIDANCE_LEN = 6 floats q[0..5] an observation can carry.
 * For an agent on p with goal g and D = d(p -> g), positions and goals being what mapf_get_state reports:
 *   q[a], a = 1 .. 4 (UP, RIGHT, DOWN, LEFT): 1.0f if D > 0 and the target cell of action a is inside the grid, is no obstacle
 *                     and has d(target -> g) = D - 1; otherwise 0.0f.  Exactly the candidate set of mapf_expert_actions mode 0:
 *                     its action is the lowest a with q[a] = 1, or 0.
 *   q[0]:             1.0f if D == 0 (the agent stands on its goal), else 0.0f
 *   q[5]:             D < 0 ? -1.0f : (float)D / (float)(H * W), the correctly rounded fp32 quotient (as goal_delta's)
 * D < 0 (no path, or p or g on an obstacle or outside the grid) gives q[0..4] = 0 and q[5] = -1.
 * (The grid graph is bipartite: a free neighbour of p is at D - 1 or D + 1, never D, so the set the search holds before its
 * last expansion decides all four bits and no second search is made.)
 * With L = mapf_obs_len of the handle's config, row (b, j) of `out` is obs[b][j][0 .. L - tail), then q[0..5], then
 * obs[b][j][L - tail .. L), the observation words copied bit for bit: out is [B][N][L + 6].  tail = 5 keeps the action mask of
 * a MAPF_FLAG_ACTION_MASK observation the last five floats of the row (where the policy kernels read it), tail = 0 appends
 * the six floats.  obs = NULL (then tail must be 0) writes the six floats alone: out is [B][N][6].
 * The shortest-path planner's contract: exactly one launch, asynchronous on `stream`, no allocation, workspace or
 * synchronisation (graph-capturable from a process's first call), no generator, a pure function of grids, positions and goals:
 * mapf_get_state before and after is identical.  It writes the B N (L + 6) (or B N 6) floats of out and nothing else, and
 * reads nothing outside obs[B][N][L] and the handle.
 * MAPF_ERR_CONFIG, and nothing is launched: a null handle or out, tail outside [0, L], tail != 0 with a null obs, out
 * overlapping obs, a MAPF_FLAG_SINGLE_AGENT handle (its observation holds the whole grid).  MAPF_ERR_STATE: before
 * mapf_set_grids. */
#define MAPF_GUIDANCE_LEN 6
int mapf_observe_guided(mapf_handle h, const float *obs /* device [B][N][L] or NULL */, int32_t tail,
                        float *out /* device [B][N][L + 6]; [B][N][6] when obs is NULL */, void *stream);

/* K independent queries on the envs' own grids: out[k] = d(env_ids[k], src[k] -> dst[k]); src / dst are (row, col).
 * Writes out[k] for every k with a valid env id (and the error record otherwise); nothing else. */
int mapf_path_lengths(mapf_handle h, int32_t K, const int32_t *env_ids /* device [K] */, const int16_t *src /* device [K][2] */,
                      const int16_t *dst /* device [K][2] */, int32_t *out /* device [K] */, void *stream);

/* field[k][r][c] = d(env_ids[k], (r, c) -> dst[k]) as uint16, 0xFFFF where it is -1 (obstacles included).
 * Writes all H * W elements of field[k] for every k with a valid env id (and the error record otherwise); nothing else. */
int mapf_distance_field(mapf_handle h, int32_t K, const int32_t *env_ids /* device [K] */, const int16_t *dst /* device [K][2] */,
                        uint16_t *field /* device [K][H][W] */, void *stream);

/* Prioritised planner: one collision-free joint plan per env, on the device (handles of either kind; the guarantee below
 * is claimed for multi-agent handles).
 * The env moves its agents in index order within a step: agent i moves before agent j > i, and a move succeeds when the
 * target cell is free at that moment (MA-env:502-526).  The planner plans the agents in that order, j = 0 .. N - 1, each in
 * space-time against the cells the ones before it occupy; with the move order as the priority order one vertex mask per
 * time step covers every conflict and no edge constraint is needed.
 * Per env, with T = horizon, times 0 .. T, p_j / g_j the cell and the goal of agent j as mapf_get_state reports them,
 * delta(a) the move of action a (0 wait, 1 UP, 2 RIGHT, 3 DOWN, 4 LEFT) and free the cells that are no obstacle:
 *   occ[t], t = 0 .. T + 1    the cells agents 0 .. j - 1 occupy at time t under their plans; occ[T + 1] := occ[T]
 *   blocked_j[t] = occ[t] | occ[t + 1], t = 0 .. T; blocked_j[1] also holds p_k of every k > j (those agents have not
 *                             moved when j makes its first move).  occ[t]: sharing a cell; occ[t + 1]: standing where an
 *                             earlier agent is about to enter, swaps included.  Following an earlier agent into the cell it
 *                             leaves in the same step is allowed, as the env allows it.
 *   reach_j[0] = {p_j};  reach_j[t] = (reach_j[t - 1] and its four neighbours) & free & ~blocked_j[t]
 *   A_j                       the smallest t <= T with g_j in reach_j[t] and g_j in no blocked_j[t'], t' = t .. T: the agent
 *                             parks on its goal from A_j on, so no earlier plan may need the goal later.  No such t (or p_j
 *                             or g_j outside the grid): the agent FAILS -- A_j = -1, all its actions are 0, and it occupies
 *                             p_j at every time for the agents after it.
 *   path                      c_{A_j} = g_j; for t = A_j .. 1: a_t = the lowest action id in 0 .. 4 with c_t - delta(a_t) in
 *                             reach_j[t - 1], c_{t-1} = c_t - delta(a_t).  plan[t - 1][j] = a_t, the steps from A_j on are 0;
 *                             occ[t] gains c_t for t <= A_j and g_j after that.
 * An env is SOLVED when every A_j >= 0.  For a solved env of a multi-agent handle, stepping the env with plan[0], plan[1], ...
 * no move fails and agent j stands on c_t after step t; every agent is on its goal after step max_j A_j at the latest.
 * Planning in a fixed order is incomplete: an env some other order, or CBS, would solve can come out unsolved.
 *
 * mapf_plan_prioritized writes all horizon * N bytes of plan[b] and all N values of arrival[b] (A_j) of every env b whose
 * mask byte is non-zero (mask NULL: every env); nothing else the caller sees.  Like the calls above it is a pure function
 * of grids, positions and goals: asynchronous on `stream`, one launch, no synchronisation, no generator, nothing the step
 * kernels read is written.  The handle keeps a workspace of B * (horizon + 1) * G * 8 bytes (G: the power of two >= H, at
 * least 4) that grows with the largest horizon asked for: a call with a horizon no larger than an earlier call's allocates
 * nothing and is graph-capturable; a larger one frees and allocates (and waits for the device), so call once before
 * capturing.  The workspace is the handle's only hidden state of a planner call: calls of one handle must be ordered on
 * one stream (or by events) -- two in flight at once share it, and a growing call frees it under the other.  It is sized
 * for every env whatever the mask selects: 270 MB at 8 192 envs x 32 rows x horizon 128, 4.3 GB at 65 536 envs x 32 rows x
 * horizon 256; plan large batches with the horizon they need.  MAPF_ERR_CONFIG: null handle, plan or arrival, horizon < 1 or > MAPF_PLAN_MAX_HORIZON(H) -- nothing is
 * launched.  MAPF_ERR_STATE: before mapf_set_grids.  mapf_plan_max_horizon returns MAPF_PLAN_MAX_HORIZON of the handle's
 * grid height (0 for a null handle). */
int mapf_plan_prioritized(mapf_handle h, int32_t horizon, const uint8_t *mask /* device [B] or NULL: all */,
                          int8_t *plan /* device [B][horizon][N] */, int32_t *arrival /* device [B][N] */, void *stream);
int mapf_plan_max_horizon(mapf_handle h);

/* Windowed prioritised planner: the next `window` steps of every env planned together, on the device (handles of either
 * kind; the guarantee below is claimed for multi-agent handles).  Rolling-horizon planning for lifelong mode, where goals
 * change under a whole-episode plan: plan w steps, play h <= w of them, plan again.  The agents are planned in the env's
 * move order against each other exactly as above, but only w steps deep, and instead of arriving an agent ends the window
 * on the cell nearest to its goal.
 * Per env, with w = window, times 0 .. w, agents planned in index order j = 0 .. N - 1 (the env's move order), p_j / g_j
 * the cell and the goal of agent j as mapf_get_state reports them, free, delta(a) and d(x -> g) as defined for the
 * shortest-path planner (-1: no path):
 *   occ[t], t = 0 .. w + 1    the cells agents 0 .. j - 1 occupy at time t under their window plans; occ[w + 1] := occ[w]
 *   blocked_j[t] = occ[t] | occ[t + 1]; blocked_j[1] also holds p_k of every k > j (the prioritised planner's rule)
 *   reach_j[0] = {p_j}, empty if p_j is outside the grid
 *   reach_j[t] = (reach_j[t - 1] and its four neighbours) & free & ~blocked_j[t], t = 1 .. w
 *   FAIL                      some reach_j[t] is empty: remaining_j = -1, arrival_j = -1, all its actions are 0, and the agent
 *                             occupies p_j at every time for the agents after it
 *   end cell                  c_w = the cell x of reach_j[w] with the smallest key (d(x -> g_j), row, col), d = -1 counting
 *                             as larger than any distance (also when g_j is outside the grid);
 *                             remaining_j = d(c_w -> g_j), or -2 where that is -1
 *   path                      for t = w .. 1: a_t = the lowest action id in 0 .. 4 with c_t - delta(a_t) in reach_j[t - 1],
 *                             c_{t-1} = c_t - delta(a_t).  plan[t - 1][j] = a_t.  Wait is id 0, so an agent that can hold its
 *                             goal to the end of the window arrives as early as it can hold it, and then waits
 *   arrival_j                 the first t in 0 .. w with c_t = g_j, -1 when there is none
 * An env is CONSISTENT when no agent fails.  For a consistent env of a multi-agent handle, in finite or lifelong mode,
 * stepping the env with plan[0], ..., plan[w - 1] no move fails and agent j stands on c_t after step t.  In lifelong mode the
 * agent's goal respawns in the step it arrives; the rest of its window (waiting) stays collision-free, so replanning at
 * that step is an improvement and never a necessity.  There is no parking condition beyond the window: agents that have
 * not arrived simply stand on c_w.
 *
 * mapf_plan_windowed writes all window * N bytes of plan[b], all N values of arrival[b] and all N values of remaining[b] of
 * every env b whose mask byte is non-zero (mask NULL: every env); nothing else.  A pure function of grids, positions and
 * goals: exactly one launch, asynchronous on `stream`, no allocation and no synchronisation ever (graph-capturable from the
 * first call), no generator, nothing the step kernels read is written.  Everything the kernel needs lives in the
 * workgroup's LDS, so the handle keeps no hidden state of the call and two calls may be in flight at once.  A workgroup
 * none of whose envs the mask selects returns before it plans anything.  MAPF_ERR_CONFIG: null handle, plan, arrival or
 * remaining, window < 1 or > MAPF_PLAN_MAX_WINDOW -- nothing is launched.  MAPF_ERR_STATE: before mapf_set_grids.
 * mapf_plan_max_window returns MAPF_PLAN_MAX_WINDOW (0 for a null handle). */
int mapf_plan_windowed(mapf_handle h, int32_t window, const uint8_t *mask /* device [B] or NULL: all */,
                       int8_t *plan /* device [B][window][N] */, int32_t *arrival /* device [B][N] */,
                       int32_t *remaining /* device [B][N] */, void *stream);
int mapf_plan_max_window(mapf_handle h);

/* Conflict-based search: the joint plan of least sum of costs per env within a horizon and a node budget, on the device
 * (handles of either kind; the guarantees below are claimed for multi-agent handles).
 * Per env, with T = horizon, times 0 .. T, p_j / g_j the cell and the goal of agent j as mapf_get_state reports them, and
 * free, delta(a) and the move order (agent i moves before k > i; a move succeeds when its target is free at that moment)
 * as defined for the planners above:
 *   constraint (a, x, t), 1 <= t <= T: agent a is not on cell x at time t.
 *   LOW LEVEL of agent a under its constraint set C_a; it ignores the other agents entirely:
 *     reach[0] = {p_a}, empty when p_a or g_a is outside the grid
 *     reach[t] = (reach[t - 1] and its four neighbours) & free & ~{x : (a, x, t) in C_a}
 *     A_a      = the smallest t <= T with g_a in reach[t] and no (a, g_a, t') in C_a for any t' >= t: the agent parks on its
 *                goal from A_a on.  No such t: the low level FAILS.
 *     path     c_{A_a} = g_a; for t = A_a .. 1: a_t = the lowest action id in 0 .. 4 with c_t - delta(a_t) in reach[t - 1],
 *                c_{t-1} = c_t - delta(a_t) (the prioritised planner's walk); c_t = g_a for t > A_a.
 *   FIRST CONFLICT of a joint plan: scan t = 0 .. T; at each t kind V before kind O; within a kind the pairs i < k in
 *   lexicographic order:
 *     V (t >= 1):     c_i[t] == c_k[t] = x.        Child constraints, in order: (i, x, t), then (k, x, t).
 *     O (t <= T - 1): c_i[t + 1] == c_k[t] = x: the later agent stands where the earlier one enters, swaps are the case
 *                     c_k[t + 1] == c_i[t].          Child constraints, in order: (i, x, t + 1), then (k, x, t).
 *     A child whose constraint would sit at time 0 is not created (it is skipped before the budget is looked at).
 *     Following an earlier agent into the cell it leaves is no conflict, as in the env; so every constraint is a vertex
 *     constraint and there are no edge constraints.
 *   HIGH LEVEL: nodes are numbered in creation order.  Node 0 holds every agent's unconstrained path; if some agent's low
 *   level fails there the status is MAPF_CBS_NO_PATH.  A node's cost is the sum of its A_j.  Repeat:
 *     1. take the open node with the smallest (cost, node id); none left: MAPF_CBS_INFEASIBLE (within T)
 *     2. it has no conflict: MAPF_CBS_SOLVED, and this node's paths are the plan
 *     3. otherwise, for each of the two child constraints in order: if max_nodes nodes exist already the status is
 *        MAPF_CBS_BUDGET, stop; replan only the constrained agent, under the constraints of the node's chain plus the new
 *        one; if that low level fails no node is created, otherwise the child joins the open list.
 * The low level is exact under its constraints and the two children of a conflict cover every conflict-free plan, so a
 * SOLVED plan has the least sum of costs (sum of A_j) of all conflict-free plans within T.
 * Guarantees.  A SOLVED env of a multi-agent handle executes its plan without a failed move, and agent j stands on c_t
 * after step t.  Every plan of mapf_plan_prioritized at the same horizon is conflict-free under V and O, so where both calls
 * solve an env the sum of costs of mapf_plan_cbs is not larger.
 *
 * mapf_plan_cbs writes, for every env b whose mask byte is non-zero (mask NULL: every env), all horizon * N bytes of plan[b],
 * all N values of arrival[b] (A_j), status[b] and nodes[b] (nodes created, the root included; 0 for NO_PATH); nothing else
 * the caller sees.  Unless status[b] is SOLVED every plan byte is 0 and every arrival is -1.  Like the planners above it is a
 * pure function of grids, positions and goals: asynchronous on `stream`, one launch, no synchronisation, no generator,
 * nothing the step kernels read is written.
 * Limits.  MAPF_CBS_MAX_HORIZON and MAPF_CBS_MAX_NODES bound the LDS tables of an env: its joint plan, N paths of P =
 * (horizon + 2 rounded up to a multiple of 4) 2-byte cells; 12 bytes per node (parent, constraint, cost key); 2 bytes per time
 * step.  At 64 agents, horizon 128 and 1 024 nodes that is 16 896 + 12 288 + 264 bytes, so at these limits every env fits
 * the 64 KiB of a workgroup and the node tables bind everywhere but at the largest agent counts; a wavefront plans as many of
 * its 64 / G envs at once as fit together.  mapf_plan_cbs_max_nodes returns the largest max_nodes that fits at
 * MAPF_CBS_MAX_HORIZON on the handle's shape (0 for a null handle).
 * Workspace.  The node store is a workspace of the handle, apart from mapf_plan_prioritized's: per env max_nodes records of
 * 16 + 2 * P bytes (parent, constraint, cost, arrival; the replanned agent's path), the N root paths (2 * N * P bytes) and the
 * reach sets of the search under way ((horizon + 1) * G * 8 bytes); mapf_plan_cbs_workspace_bytes gives the total for B envs
 * (0 for arguments the call refuses).  It follows that workspace's rules: it grows with the largest need asked for, a call
 * that needs no more than an earlier one allocates nothing and is graph-capturable, a larger one frees and allocates (and
 * waits for the device), so call once before capturing; calls of one handle must be ordered on one stream.
 * MAPF_ERR_CONFIG: a null handle or buffer, horizon outside [1, MAPF_CBS_MAX_HORIZON], max_nodes outside [1,
 * MAPF_CBS_MAX_NODES], or tables of one env beyond 64 KiB of LDS -- nothing is launched and nothing falls back.
 * MAPF_ERR_STATE: before mapf_set_grids. */
#define MAPF_CBS_SOLVED 0
#define MAPF_CBS_BUDGET 1
#define MAPF_CBS_INFEASIBLE 2
#define MAPF_CBS_NO_PATH 3
int mapf_plan_cbs(mapf_handle h, int32_t horizon, int32_t max_nodes, const uint8_t *mask /* device [B] or NULL: all */,
                  int8_t *plan /* device [B][horizon][N] */, int32_t *arrival /* device [B][N] */, int32_t *status /* device [B] */,
                  int32_t *nodes /* device [B] */, void *stream);
int mapf_plan_cbs_max_nodes(mapf_handle h);
int64_t mapf_plan_cbs_workspace_bytes(mapf_handle h, int32_t horizon, int32_t max_nodes);

/* Fused recurrent policy: observation to action, log-probability, value and new LSTM state in one launch, for every agent
 * of every env (the policies the reference trains, src/agents/ppo.py:67-75 and impala.py:54-59: 64-64 dense plus an LSTM
 * of 64 that also sees the previous action and reward, behind models/action_mask_model.py).
 * A policy handle is independent of an env handle.  It works on `rows` agent rows, rows = B * N; agents_per_env = N maps a
 * row to its env (env = row / N).  The hidden width is MAPF_POLICY_HIDDEN = 64, the reference's size (a compile-time
 * parameter of the kernel, so other widths can be added later); any other `hidden` is MAPF_ERR_CONFIG.
 * Config: obs_len = L in [1, the longest observation mapf_obs_len can return = 130]; mask_off = -1, or L - 5 when the
 * observation ends in the 5-float action mask; recurrent 0 or 1; agents_per_env >= 1; device.  The feature count is
 * F = mask_off when a mask is present, otherwise L.
 * Per row, everything in fp32:
 *   x   = obs[row][0 .. F)
 *   a1  = tanh(W1 x + b1)                 W1 [64][F]
 *   a2  = tanh(W2 a1 + b2)                W2 [64][64]
 *   recurrent:  z = [a2, onehot5(prev_action), prev_reward]          (70 inputs)
 *               torch.nn.LSTMCell semantics, gate order i, f, g, o:
 *               g = Wih z + bih + Whh h + bhh;  c' = sig(f) c + sig(i) tanh(g_g);  h' = sig(o) tanh(c')
 *               u = h'
 *   otherwise:  u = a2
 *   logits = Wp u + bp  [+ log(mask + 1e-6) when mask_off >= 0]      (models/action_mask_model.py:52-64; its clamp never binds)
 *   value  = Wv u + bv
 *   action = argmax_k (logits[k] + g_k), lowest k on ties;  g_k = 0 in greedy mode, Gumbel noise in sample mode
 *   logp   = log_softmax(logits)[action]
 * Episode start: a row whose env has a non-zero byte in either of the two optional device flag arrays start_a[B] and
 * start_b[B] uses h = c = 0, prev_action = 0 and prev_reward = 0 for this call (two arrays, so that a step's `terminated`
 * and `truncated` can be passed as they are, with no OR launch in between).  A NULL prev_action or prev_reward means zeros.
 * prev_action is int8 [rows]; a byte outside 0 .. 4 contributes no one-hot entry.
 * Noise: counter-based, by the splitmix64 finalizer `mix` of the masked-random policy of the fused step launches:
 *   x   = mix(seed ^ ((uint64)row << 32 | draws[row]))
 *   x_k = mix(x + (k + 1) * 0x9E3779B97F4A7C15)
 *   u_k = ((x_k >> 40) + 0.5) * 2^-24
 *   g_k = -log(-log(u_k))                  (evaluated in double and added to the fp32 logit in double: u_k has 25 bits)
 * draws[rows] (uint32) is per-row state like h and c: each row reads its own counter and stores it plus one, so a captured
 * graph draws fresh noise on every replay without a host-side counter.  Greedy mode neither reads nor writes draws.
 * Precision is part of the rule: fp32 operands with fp32 accumulation on the f32-input matrix instruction
 * (v_mfma_f32_32x32x2_f32), any summation order; bias sums such as bih + bhh may be formed first.  bf16, fp16 and
 * split-bf16 operands are out of scope: on logits of size 0.1 to 0.3 they leave 2-9 % of the greedy decisions within the
 * rounding noise, and a rollout's logp would no longer be the learner's.
 *
 * Parameters: the flat fp32 vector in the state_dict order of policy.MaskedRecurrentPolicy:
 *   fc1.weight [64][F], fc1.bias, fc2.weight [64][64], fc2.bias, [lstm.weight_ih [256][70], lstm.weight_hh [256][64],
 *   lstm.bias_ih, lstm.bias_hh,] pi.weight [5][64], pi.bias, vf.weight [1][64], vf.bias
 * mapf_policy_param_count returns its length (0 for a null handle).  mapf_policy_set_params is asynchronous on `stream`:
 * one launch that rewrites the weights into the layout the act kernel reads (zero-padded to the matrix instruction's K), no
 * synchronisation, so a learner can push weights every iteration; MAPF_ERR_CONFIG for a null argument or another count.
 * Mode: bit 0 MAPF_POLICY_SAMPLE; bit 1 MAPF_POLICY_PEEK: every output is computed but hstate, cstate and draws are not
 * written (a rollout's bootstrap value).  logp, value and logits may be NULL.  prev_action may alias action: a row is read
 * before it is written.  hstate and cstate are 16-byte aligned.
 * Contract: exactly one launch, asynchronous on `stream`; no allocation, no synchronisation and no workspace; graph-
 * capturable from the first call; two calls on different state may be in flight at once.  mapf_policy_act writes the `rows`
 * elements of each non-NULL output and, unless PEEK, of hstate / cstate (recurrent) and draws (sample mode), and nothing
 * else, also when rows is not a multiple of the kernel's 32-row tile.  It never reads outside obs[rows][L] or any [rows]
 * array; the zero-padded K tail of the first product is not fed from memory.  MAPF_ERR_CONFIG: a null handle, obs or action,
 * null hstate or cstate (when recurrent), null draws (when sampling), rows < 1, rows not a multiple of agents_per_env while
 * a start flag array is given, unknown mode bits.  MAPF_ERR_STATE: before mapf_policy_set_params.  Nothing is launched in
 * either case. */
#define MAPF_POLICY_HIDDEN 64
#define MAPF_POLICY_SAMPLE 1
#define MAPF_POLICY_PEEK 2
typedef struct mapf_policy_config {
    int32_t obs_len;        /* L */
    int32_t mask_off;       /* -1, or L - 5 */
    int32_t recurrent;      /* 0 or 1 */
    int32_t agents_per_env; /* N: env of a row = row / N */
    int32_t hidden;         /* MAPF_POLICY_HIDDEN */
    int32_t device;
} mapf_policy_config;
typedef struct mapf_policy *mapf_policy_handle;
int mapf_policy_create(const mapf_policy_config *cfg /* host */, mapf_policy_handle *out);
int mapf_policy_destroy(mapf_policy_handle h);
int64_t mapf_policy_param_count(mapf_policy_handle h);
int mapf_policy_set_params(mapf_policy_handle h, const float *params /* device, flat */, int64_t count, void *stream);
int mapf_policy_act(mapf_policy_handle h, int32_t rows, const float *obs /* device [rows][L] */,
                    const int8_t *prev_action /* device [rows] or NULL */, const float *prev_reward /* device [rows] or NULL */,
                    const uint8_t *start_a /* device [B] or NULL */, const uint8_t *start_b /* device [B] or NULL */,
                    float *hstate, float *cstate /* device [rows][64], in/out */, uint32_t *draws /* device [rows], in/out */,
                    uint64_t seed, int32_t mode, int8_t *action /* device [rows] */, float *logp, float *value /* device [rows] */,
                    float *logits /* device [rows][5] */, void *stream);

/* One policy per agent (the reference's training_execution_mode "DTE", src/agents/ppo.py:77-88: policies = {agent_i:
 * PolicySpec()}, policy_mapping_fn = agent_id).  mapf_policy_create_per_agent takes the same config and returns a handle of
 * the same type that holds P = agents_per_env weight sets, P in [1, MAPF_MAX_AGENTS] (anything else: MAPF_ERR_CONFIG); row
 * r is computed with set r % P by the rule above, so rows b * P + a of the usual [B][N] layout belong to agent a.
 * mapf_policy_param_count returns P times the per-policy count; mapf_policy_set_params takes the concatenation
 * [P][per-policy vector], policy-major, each policy in the state_dict order above (the flat vector of
 * policy.PerAgentPolicy), and packs all P sets in one launch, asynchronous and repeatable as above.  mapf_policy_act,
 * _destroy and _param_count are the calls above.  On such a handle rows must be a multiple of P whether or not start
 * flags are given (MAPF_ERR_CONFIG, nothing launched).  The launch: a 32-row tile of the matrix instruction holds 32 ENVS
 * of one agent (lane j of tile (a, eb) owns row (32 eb + j) P + a), the grid is P * ceil(B / 32) one-wave workgroups, and
 * only the addressing differs from the shared launch: the arithmetic of a row does not depend on its tile-mates, so row r
 * gets bit for bit what a shared handle with set r % P returns for it on the same inputs and state; the noise is that of
 * the global row index.  Everything else (modes, NULL outputs, aliasing, what is read and written, graph capture) is
 * the contract above. */
int mapf_policy_create_per_agent(const mapf_policy_config *cfg /* host */, mapf_policy_handle *out);

/* Any map from rows to weight sets that repeats every `groups` rows (a population of P policies trained side by side on
 * one env handle: env b belongs to member b % P, so with N agents per env groups = P N and set_of_group[g] = g / N; the
 * reference's tuner, src/trainers/tuner.py, runs such a population as separate trials).  mapf_policy_create_mapped takes the
 * config above and returns a handle of the same type that holds `sets` weight sets; row r is computed with set
 * set_of_group[r % groups] by the rule above.  groups is a positive multiple of cfg->agents_per_env, at most
 * MAPF_POLICY_MAX_GROUPS; 1 <= sets <= groups; every entry of the host array set_of_group[groups] lies in [0, sets);
 * anything else is MAPF_ERR_CONFIG and nothing is created.  The map is copied into device memory the handle owns, once, at
 * creation (a synchronous copy: creation is no part of a captured graph).  agents_per_env keeps its meaning: the env of a
 * row is row / agents_per_env, for the start flags.  mapf_policy_param_count returns `sets` times the per-policy count;
 * mapf_policy_set_params takes [sets][per-policy vector], set-major, and packs all sets in one launch.  On such a handle rows
 * must be a multiple of groups whether or not start flags are given (MAPF_ERR_CONFIG, nothing launched).  The launch is the
 * per-agent one with groups in the place of P: a tile holds 32 UNITS of one group g (lane j of tile (g, ub) owns row
 * (32 ub + j) groups + g), the grid is groups * ceil(rows / groups / 32) one-wave workgroups, group-major, and a workgroup
 * reads its group's map entry once.  Row r gets bit for bit what a shared handle loaded with set set_of_group[r % groups]
 * returns for it on the same inputs and state; the noise is that of the global row index.  A per-agent handle IS the
 * mapped handle with groups = sets = agents_per_env and the identity map.  Everything else is the contract above. */
#define MAPF_POLICY_MAX_GROUPS 1024
int mapf_policy_create_mapped(const mapf_policy_config *cfg /* host */, int32_t groups, int32_t sets,
                              const int32_t *set_of_group /* host [groups] */, mapf_policy_handle *out);

/* Joint-action policy of the single-agent env (the reference's training_execution_mode "CTE", src/agents/ppo.py:25-64
 * behind models/action_mask_model_single.py): one policy moves all N agents of an env, the observation is the full grid,
 * the action is MultiDiscrete([5] * N).  A sibling of the fused recurrent policy above: the same network (64-64 dense plus
 * an LSTM of 64 that also sees the previous action and reward), the same noise, modes and precision rule, on env rows.
 * A handle is independent of an env handle.  One row is one env.  F = grid_cells = H * W, N = num_agents, L = F + 5 N is
 * mapf_obs_len of the single-agent env; the action mask is always the last 5 N floats and is no feature.
 * Config: grid_cells in [1, MAPF_JPOLICY_MAX_CELLS = 4096]; num_agents in [1, MAPF_JPOLICY_MAX_AGENTS = 64]; recurrent 0
 * or 1; hidden = MAPF_POLICY_HIDDEN, or MAPF_JPOLICY_HIDDEN_WIDE = 256 with recurrent = 0 (the wide net, below); device.
 * Anything else is MAPF_ERR_CONFIG, a recurrent wide net and every other width included.
 * Per row, everything in fp32 with fp32 accumulation, in any summation order:
 *   x      = obs[row][0 .. F)
 *   a1     = tanh(W1 x + b1)                 W1 [64][F]
 *   a2     = tanh(W2 a1 + b2)                W2 [64][64]
 *   recurrent:  z = [a2, onehot5(prev_action[row][0]), ..., onehot5(prev_action[row][N-1]), prev_reward]   (64 + 5 N + 1 inputs)
 *               torch.nn.LSTMCell semantics, gate order i, f, g, o;  u = h'
 *   otherwise:  u = a2
 *   logits = Wp u + bp + log(obs[row][F .. F + 5 N) + 1e-6)          [5 N]
 *   value  = Wv u + bv
 *   action[row][i] = argmax_k (logits[5 i + k] + g_{i,k}), lowest k on ties;  g = 0 in greedy mode
 *   logp[row]      = sum_i log_softmax(logits[5 i .. 5 i + 5))[action[row][i]]
 * Noise: one draw counter per row, as above:
 *   x       = mix(seed ^ ((uint64)row << 32 | draws[row]))
 *   x_{i,k} = mix(x + (5 i + k + 1) * 0x9E3779B97F4A7C15)
 *   u_{i,k} = ((x_{i,k} >> 40) + 0.5) * 2^-24;   g_{i,k} = -log(-log(u_{i,k})), in double
 * For N = 1 this is the noise of mapf_policy_act.  Sample mode reads draws[row] and, unless PEEK, stores it plus one.
 * prev_reward is const double [rows], rounded to nearest fp32 on load, so the reward array mapf_cte_step writes can be
 * passed as it is; prev_action is int8 [rows][N], and a byte outside 0 .. 4 contributes no one-hot entry.  A NULL
 * prev_action or prev_reward means zeros (action 0, reward 0).
 * Episode start: start_a / start_b are optional uint8 [rows] device arrays; a row with a non-zero byte in either uses
 * h = c = 0, zero previous actions and a zero previous reward for this call.
 * Parameters: the flat fp32 vector in the state_dict order of policy.JointActionPolicy:
 *   fc1.weight [64][F], fc1.bias, fc2.weight [64][64], fc2.bias, [lstm.weight_ih [256][64 + 5 N + 1], lstm.weight_hh
 *   [256][64], lstm.bias_ih, lstm.bias_hh,] pi.weight [5 N][64], pi.bias [5 N], vf.weight [1][64], vf.bias
 * mapf_jpolicy_param_count returns its length (0 for a null handle).  mapf_jpolicy_set_params is asynchronous on `stream`:
 * one launch that rewrites the weights into the layout the act kernel reads, no synchronisation; MAPF_ERR_CONFIG for a
 * null argument or another count.
 * Mode: MAPF_POLICY_SAMPLE and MAPF_POLICY_PEEK with their meaning above.  Outputs: action int8 [rows][N]; logp, value
 * [rows]; logits [rows][5 N]; the last three may be NULL.  prev_action may alias action: a row is read before it is
 * written.  hstate and cstate are [rows][64], 16-byte aligned.
 * The wide net (hidden = MAPF_JPOLICY_HIDDEN_WIDE, feed-forward only) is the reference's CTE IMPALA model
 * (src/agents/impala.py:16-51: fcnet_hiddens = [256, 256], no LSTM).  Its per-row rule is the one above with W1 [256][F],
 * W2 [256][256], u = a2, Wp [5 N][256] and Wv [1][256]: the same tanh and log(mask + 1e-6), the same argmax / Gumbel-max
 * with the same noise and the lowest k on ties, the same summed log-probability, modes, NULL outputs, aliasing rule and
 * precision rule.  The value head sits on the shared trunk, as in every net here: RLlib's default model config shares
 * the value layers (vf_share_layers) unless told otherwise, and the reference's CTE IMPALA config does not say
 * otherwise.  Its parameters are the state_dict order of policy.JointActionPolicy(F, N, recurrent=False, hidden=256):
 *   fc1.weight [256][F], fc1.bias, fc2.weight [256][256], fc2.bias, pi.weight [5 N][256], pi.bias, vf.weight [1][256], vf.bias
 * A feed-forward handle of either width reads neither prev_action, prev_reward, the start flags nor hstate / cstate, all
 * of which may be NULL.  The same entry points serve both widths, and so does the contract below.
 * Contract: exactly one launch, asynchronous on `stream`; no allocation, no synchronisation and no workspace; graph-
 * capturable from a process's first call.  mapf_jpolicy_act writes the `rows` elements of each non-NULL output and, unless
 * PEEK, of hstate / cstate (recurrent) and draws (sample mode), and nothing else, also when rows is not a multiple of the
 * kernel's 32-row tile.  It never reads outside obs[rows][L] or any [rows] array; the zero-padded K tails of the products
 * are not fed from memory.  MAPF_ERR_CONFIG: a null handle, obs or action, null hstate or cstate (when recurrent), null
 * draws (when sampling), rows < 1, unknown mode bits.  MAPF_ERR_STATE: before mapf_jpolicy_set_params.  Nothing is
 * launched in either case. */
#define MAPF_JPOLICY_MAX_CELLS 4096
#define MAPF_JPOLICY_MAX_AGENTS 64
#define MAPF_JPOLICY_HIDDEN_WIDE 256
typedef struct mapf_jpolicy_config {
    int32_t grid_cells; /* F = H * W */
    int32_t num_agents; /* N */
    int32_t recurrent;  /* 0 or 1 */
    int32_t hidden;     /* MAPF_POLICY_HIDDEN, or MAPF_JPOLICY_HIDDEN_WIDE with recurrent = 0 */
    int32_t device;
} mapf_jpolicy_config;
typedef struct mapf_jpolicy *mapf_jpolicy_handle;
int mapf_jpolicy_create(const mapf_jpolicy_config *cfg /* host */, mapf_jpolicy_handle *out);
int mapf_jpolicy_destroy(mapf_jpolicy_handle h);
int64_t mapf_jpolicy_param_count(mapf_jpolicy_handle h);
int mapf_jpolicy_set_params(mapf_jpolicy_handle h, const float *params /* device, flat */, int64_t count, void *stream);
int mapf_jpolicy_act(mapf_jpolicy_handle h, int32_t rows, const float *obs /* device [rows][L] */,
                     const int8_t *prev_action /* device [rows][N] or NULL */, const double *prev_reward /* device [rows] or NULL */,
                     const uint8_t *start_a /* device [rows] or NULL */, const uint8_t *start_b /* device [rows] or NULL */,
                     float *hstate, float *cstate /* device [rows][64], in/out */, uint32_t *draws /* device [rows], in/out */,
                     uint64_t seed, int32_t mode, int8_t *action /* device [rows][N] */, float *logp, float *value /* device [rows] */,
                     float *logits /* device [rows][5 N] */, void *stream);

/* LSTM recurrence over a whole fragment, forward and backward: the sequential part of a learner's pass over T steps of
 * `rows` agent rows, one launch each (the dense layers, the input half of the gates and the heads do not depend on the
 * recurrence and are the caller's, evaluated for all T at once).  Neither call needs a handle; the weights are passed as
 * torch stores them.  Hidden width MAPF_POLICY_HIDDEN = 64, gate order i, f, g, o.
 * Per row, everything in fp32 with torch.nn.LSTMCell semantics, for t = 0 .. T - 1:
 *   (hp, cp) = (0, 0) where reset[t][row] != 0, otherwise (h[t-1], c[t-1]), (h0, c0) at t = 0
 *   G        = xg[t] + Whh hp                       xg[t] = Wih z_t + bih + bhh, computed by the caller
 *   i, f, o  = sig(G_i), sig(G_f), sig(G_o);  g = tanh(G_g)
 *   c[t]     = f cp + i g;   h[t] = o tanh(c[t]);   gates[t] = [i, f, g, o] (activated, kept for backward)
 * Backward takes dh[t] = dLoss/dh[t] of every step (from the heads) and the gradient that arrives at the final state
 * (dhT, dcT; NULL: zeros), and returns dxg[t] = dLoss/dG_t, dh0 and dc0:
 *   dH = dh[t] + (Whh^T dxg[t+1], or dhT at T - 1);  dC = dH o (1 - tanh(c[t])^2) + (dC' f' of step t + 1, or dcT)
 *   dxg[t] = [dC g i (1 - i), dC cp f (1 - f), dC i (1 - g^2), dH tanh(c[t]) o (1 - o)]
 *   a set reset[t] cuts both terms that flow into step t - 1 (and into dh0 / dc0 at t = 0).
 * The weight gradient is not part of the kernel; it is one product: dWhh = sum_t dxg[t]^T hp_t.
 * Precision as for the policy: fp32 operands, fp32 accumulation on v_mfma_f32_32x32x2_f32, any summation order.  No
 * atomics: a row's results depend on that row's inputs alone and both calls are bitwise repeatable.
 * Contract: exactly one launch each, asynchronous on `stream`; no allocation, no workspace, no synchronisation; graph-
 * capturable from the first call; any T >= 1 and rows >= 1.  Forward writes h[T][rows][64], c[T][rows][64] and, unless
 * NULL, gates[T][rows][256]; backward writes dxg[T][rows][256] and, unless NULL, dh0 and dc0 [rows][64]; nothing else is
 * written, also when rows is not a multiple of the kernel's 32-row tile, and nothing outside the inputs is read.  Every
 * float pointer is 16-byte aligned.  MAPF_ERR_CONFIG: T < 1, rows < 1 or a null pointer other than reset, gates (forward),
 * dhT, dcT, dh0, dc0; nothing is launched then. */
int mapf_lstm_seq_forward(int32_t T, int32_t rows, const float *xg /* device [T][rows][256] */,
                          const float *whh /* device [256][64]: lstm.weight_hh */, const uint8_t *reset /* device [T][rows] or NULL */,
                          const float *h0, const float *c0 /* device [rows][64] */, float *h, float *c /* device [T][rows][64] */,
                          float *gates /* device [T][rows][256] or NULL */, void *stream);
int mapf_lstm_seq_backward(int32_t T, int32_t rows, const float *whh, const uint8_t *reset, const float *c0, const float *c,
                           const float *gates, const float *dh /* device [T][rows][64] */,
                           const float *dhT, const float *dcT /* device [rows][64] or NULL */, float *dxg /* device [T][rows][256] */,
                           float *dh0, float *dc0 /* device [rows][64] or NULL */, void *stream);

/* The same two calls with `groups` recurrent matrices: row r recurs through whh[r % groups] (one policy per agent on the
 * interleaved agent rows b * N + a, groups = N, so a learner never permutes its [T][rows][...] tensors).  Everything else
 * is the rule and the contract above; groups < 1 or rows not a multiple of groups is MAPF_ERR_CONFIG.  A 128-row
 * workgroup stages the image of its own group and owns rows g + groups * i of it; the grid is groups * ceil(rows / groups
 * / 128).  mapf_lstm_seq_forward / _backward are groups = 1 of the same kernels, so a group's rows get bit for bit what
 * the ungrouped calls return on those rows gathered contiguously with whh[g].  The weight gradient stays the caller's: one
 * batched product, dWhh[g] = sum over t and the rows of group g of dxg[t]^T hp_t. */
int mapf_lstm_seq_forward_grouped(int32_t T, int32_t rows, int32_t groups, const float *xg /* device [T][rows][256] */,
                                  const float *whh /* device [groups][256][64] */, const uint8_t *reset, const float *h0,
                                  const float *c0, float *h, float *c, float *gates, void *stream);
int mapf_lstm_seq_backward_grouped(int32_t T, int32_t rows, int32_t groups, const float *whh /* device [groups][256][64] */,
                                   const uint8_t *reset, const float *c0, const float *c, const float *gates, const float *dh,
                                   const float *dhT, const float *dcT, float *dxg, float *dh0, float *dc0, void *stream);

/* Fused dense trunk of the learner: observation to gate inputs for a whole minibatch, forward and backward, one launch
 * each.  It is the first half of the fused recurrent policy's rule on M = T x rows gathered, contiguous rows instead of one
 * step's, with what the backward pass needs kept; the recurrence (mapf_lstm_seq_*), the heads and the objective follow it.
 * Neither call needs a handle: the weights are passed as torch stores them, row-major (fc1.weight [64][F], fc1.bias [64],
 * fc2.weight [64][64], fc2.bias [64], lstm.weight_ih [256][70], lstm.bias_ih and lstm.bias_hh [256]), because they change
 * with every optimiser step.  Scope: one net, one head, hidden width MAPF_POLICY_HIDDEN = 64, F features in 1 ..
 * MAPF_TRUNK_MAX_FEATURES, rows of L = F floats or L = F + 5 (the action mask behind the features), recurrent or
 * feed-forward.  Per row m, everything in fp32:
 *   x   = obs[m][0 .. F)                                  columns F .. L (the mask) are never read
 *   a1  = tanh(W1 x + b1);   a2 = tanh(W2 a1 + b2)
 *   recurrent:  pa, pr = first[m] ? (0, 0) : (prev_action[m], prev_reward[m])
 *               xg = Wih [a2, onehot5(pa), pr] + bih + bhh            [256], gate order i, f, g, o: what mapf_lstm_seq_forward reads
 * A prev_action byte outside 0 .. 4 adds no one-hot entry, as in mapf_policy_act.
 * Backward takes dxg [M][256] = dLoss/dxg (recurrent) or da2 [M][64] = dLoss/da2 (feed-forward) and the saved a1, a2, and
 * returns the gradients with respect to the pre-activations:
 *   dpre2 = (Wih[:, 0 .. 64)^T dxg) (1 - a2^2),  or  da2 (1 - a2^2) when feed-forward
 *   dpre1 = (W2^T dpre2) (1 - a1^2)
 * There is no gradient with respect to obs.  The parameter gradients are not part of the kernel; they are products and
 * column sums over the M rows: dWih = dxg^T [a2, onehot5(pa), pr], dW2 = dpre2^T a1, dW1 = dpre1^T x, dbih = dbhh = sum dxg,
 * db2 = sum dpre2, db1 = sum dpre1.
 * Precision as for the policy: fp32 operands, fp32 accumulation on v_mfma_f32_32x32x2_f32, any summation order, libm-grade
 * tanh.  No atomics and no sum over rows: a row's results depend on that row's inputs alone, not on M or on the row's place
 * in the launch, and both calls are bitwise repeatable.
 * Contract: exactly one launch each, asynchronous on `stream`; no allocation, no workspace, no synchronisation; graph-
 * capturable from the first call; any M >= 1, with 64-bit row and element indices.  Forward writes a1 and a2 [M][64] and,
 * when recurrent, xg [M][256]; backward writes dpre2 and dpre1 [M][64]; nothing else is written, also when M is not a
 * multiple of the kernel's 32-row tile, and nothing outside the arrays named is read: the zero K-tail of fc1 at odd F is
 * not fed from memory.  a1, a2, xg, dxg, da2, dpre2 and dpre1 are accessed 16 bytes at a time.
 * MAPF_ERR_CONFIG, and nothing is launched: M < 1; F outside 1 .. MAPF_TRUNK_MAX_FEATURES; L neither F nor F + 5; recurrent
 * neither 0 nor 1; a null obs, w1, b1, w2, b2, a1, a2 (forward) or a1, a2, w2, dpre2, dpre1 (backward); recurrent = 1 with a
 * null prev_action, prev_reward, first, wih, bih, bhh or xg (forward), a null dxg or wih or a non-null da2 (backward);
 * recurrent = 0 with a non-null xg (forward), a null da2 or a non-null dxg (backward: wih is then not read); one of the
 * arrays accessed 16 bytes at a time not 16-byte aligned. */
#define MAPF_TRUNK_MAX_FEATURES 125
int mapf_trunk_forward(int64_t M, int32_t F, int32_t L, int32_t recurrent, const float *obs /* device [M][L] */,
                       const int8_t *prev_action /* device [M] */, const float *prev_reward /* device [M] */,
                       const uint8_t *first /* device [M]; the three: recurrent only, else NULL or ignored */,
                       const float *w1, const float *b1, const float *w2, const float *b2,
                       const float *wih, const float *bih, const float *bhh /* recurrent only */,
                       float *a1, float *a2 /* device [M][64] */, float *xg /* device [M][256], or NULL when feed-forward */,
                       void *stream);
int mapf_trunk_backward(int64_t M, int32_t recurrent, const float *dxg /* device [M][256] or NULL */,
                        const float *da2 /* device [M][64] or NULL */, const float *a1, const float *a2 /* device [M][64] */,
                        const float *wih /* lstm.weight_ih, recurrent only */, const float *w2,
                        float *dpre2, float *dpre1 /* device [M][64] */, void *stream);

/* Fused parameter gradients of the learner: the sums over rows that mapf_trunk_backward and mapf_lstm_seq_backward leave to
 * the caller, as one split-row reduction on v_mfma_f32_32x32x2_f32 with the rows as the inner dimension.  No handle.
 * mapf_trunk_param_grad takes what the two trunk calls read and wrote on M contiguous rows and returns, row-major as torch
 * stores fc1.weight, fc2.weight and lstm.weight_ih (the rule is the one stated above under "Fused dense trunk of the learner"):
 *   dW1 [64][F] = dpre1^T obs[:, 0 .. F)      db1 [64] = sum dpre1
 *   dW2 [64][64] = dpre2^T a1                 db2 [64] = sum dpre2
 *   recurrent:  dWih [256][70] = dxg^T [a2, onehot5(pa), pr]      dbl [256] = sum dxg  (= dbih = dbhh)
 * with pa, pr = first[m] ? (0, 0) : (prev_action[m], prev_reward[m]) and no one-hot entry for a byte outside 0 .. 4, exactly
 * as in mapf_trunk_forward; the 70-column operand is formed in the kernel and never exists in memory, columns F .. L of obs
 * (the mask) are never read, and prev_action / prev_reward of a row with first set are selected away, whatever they hold (a
 * NaN reward there does not reach the result).  An output pointer that is
 * NULL is skipped; with dWih = dbl = NULL the four recurrent inputs and dxg are not read and may be NULL.
 * mapf_lstm_seq_param_grad takes what the grouped recurrence calls read and wrote and returns
 *   dWhh [groups][256][64]:  dWhh[g] = sum over t and the rows r with r % groups == g of dxg[t][r]^T hp[t][r]
 *   hp[0] = h0, hp[t] = h[t-1], and hp[t][r] = 0 where reset[t][r] != 0 (reset NULL: never)
 * hp is never written to memory: the kernel reads h one step back.  groups = 1 is the shared matrix.
 * Both: a workgroup reduces one contiguous slab of rows (of one group) into its own partial result in `workspace`, a second
 * launch adds the partials in slab order.  The partition depends on the shape alone, never on the device: with n the rows
 * of one group (M; T rows / groups), slabs of MAPF_PARAM_GRAD_SLAB_ROWS rows while that gives at most
 * MAPF_PARAM_GRAD_MAX_SLABS of them, otherwise slabs of ceil(n / MAPF_PARAM_GRAD_MAX_SLABS) rows rounded up to a multiple
 * of 32.  No atomics, a fixed summation order: two calls are bitwise equal.  fp32 operands and accumulation.
 * mapf_param_grad_workspace_bytes(rows, F, recurrent, groups): the bytes either call needs -- groups = 0: the trunk call on
 * M = rows (slabs x (2 ceil((F + 1) / 32) + 6 + 24 recurrent) tiles of 4 KiB: 39.8 MB at most); groups >= 1: the recurrence
 * call with rows = T x rows-per-step (groups x slabs x 64 KiB: 16.8 MB per group at most); 0 for arguments the calls refuse.
 * Contract: two launches per call (none when every output is NULL), asynchronous on `stream`; no allocation, no
 * synchronisation; graph-capturable from the first call; 64-bit row and element indices.  Exactly the outputs named and the
 * first mapf_param_grad_workspace_bytes(...) bytes of the workspace are written, nothing outside the arrays named is read,
 * and a row tail (M odd, a last slab of one row) is never loaded past row M.  a1, a2, dpre1, dpre2, dxg, h, h0 and the
 * workspace are accessed 16 bytes at a time; obs, prev_action, prev_reward, first and reset element by element.
 * MAPF_ERR_CONFIG, and nothing is launched: M < 1; T < 1; rows < 1; groups < 1, above 65535 or not dividing rows; F outside
 * 1 .. MAPF_TRUNK_MAX_FEATURES; L neither F nor F + 5; recurrent neither 0 nor 1; a null obs, a1, a2, dpre1 or dpre2 (trunk), a
 * null dxg, h, h0 or dWhh (recurrence); recurrent = 1 with a null dxg, prev_action, prev_reward or first while dWih or dbl is
 * asked for; recurrent = 0 with a non-null dWih or dbl; a workspace that is null, smaller than the query's answer or not
 * 16-byte aligned; one of the arrays accessed 16 bytes at a time not 16-byte aligned. */
#define MAPF_PARAM_GRAD_SLAB_ROWS 1024
#define MAPF_PARAM_GRAD_MAX_SLABS 256
int64_t mapf_param_grad_workspace_bytes(int64_t rows, int32_t F, int32_t recurrent, int32_t groups);
int mapf_trunk_param_grad(int64_t M, int32_t F, int32_t L, int32_t recurrent, const float *obs /* device [M][L] */,
                          const int8_t *prev_action, const float *prev_reward, const uint8_t *first /* device [M], recurrent only */,
                          const float *a1, const float *a2, const float *dpre1, const float *dpre2 /* device [M][64] */,
                          const float *dxg /* device [M][256] or NULL */, float *dw1 /* [64][F] */, float *db1 /* [64] */,
                          float *dw2 /* [64][64] */, float *db2 /* [64] */, float *dwih /* [256][70] */, float *dbl /* [256] */,
                          void *workspace, int64_t workspace_bytes, void *stream);
int mapf_lstm_seq_param_grad(int32_t T, int32_t rows, int32_t groups, const float *dxg /* device [T][rows][256] */,
                             const float *h /* device [T][rows][64] */, const float *h0 /* device [rows][64] */,
                             const uint8_t *reset /* device [T][rows] or NULL */, float *dwhh /* device [groups][256][64] */,
                             void *workspace, int64_t workspace_bytes, void *stream);

/* The IMPALA objective on a fragment: V-trace targets, the three loss terms and their gradients with respect to the
 * logits and the values, one launch (the network's forward and backward are the caller's; the targets are recomputed
 * from the current network in every learner step).  No handle.  Per row, for T steps and `heads` five-way action heads (an
 * agent row of the multi-agent env has one head; an env row of a joint fragment has N, its log-probability is the sum
 * over its agents and its entropy the sum of their entropies), everything in fp32:
 *   lp_k      = log_softmax(logits[t] of head k);  logp[t] = sum_k lp_k[a_k];  H[t] = -sum_k sum_j exp(lp_kj) lp_kj
 *   w         = exp(logp[t] - behaviour_logp[t])
 *   rho, c, rho_pg = min(clip_rho, w),  lam * min(clip_c, w),  min(clip_pg_rho, w)
 *   disc      = gamma * (ended[t] ? 0 : 1)
 *   nextV     = values[t+1]  (bootstrap at t = T-1);   nextVs = vs[t+1]  (bootstrap at t = T-1)
 *   delta     = rho * (rewards[t] + disc * nextV - values[t])
 *   acc[t]    = delta + disc * c * acc[t+1]            (acc[T] = 0)
 *   vs[t]     = values[t] + acc[t]
 *   pg_adv[t] = rho_pg * (rewards[t] + disc * nextVs - values[t])
 *   policy_loss = -mean(pg_adv * logp);  vf_loss = 0.5 * mean((values - vs)^2);  entropy = mean(H)
 *   total_loss  = policy_loss + vf_coeff * vf_loss - ent_coeff * entropy          (means over T x rows)
 * vs, pg_adv and the three weights are constants of the objective, so the gradients are closed-form:
 *   dlogits[t][k][j] = [ -pg_adv (1[j = a_k] - p_kj) + ent_coeff p_kj (lp_kj + H_k) ] / (T rows)     p = exp(lp)
 *   dvalues[t]       = vf_coeff (values[t] - vs[t]) / (T rows)
 * An episode end (ended[t] != 0) cuts the bootstrap and the recursion: the terms behind disc are left out, not multiplied
 * by 0, so a row that ends at step s equals the same row run as two calls bitwise.  A probability that underflows to 0 adds
 * 0 to the entropy and has a 0 entropy gradient (never 0 x inf); a w that overflows to +inf clips to its threshold.  An
 * action byte outside 0 .. 4 is clamped before it indexes anything.
 * partials [mapf_vtrace_partials(rows)][4]: per workgroup the sums over its (t, row) of -pg_adv logp, 0.5 (values - vs)^2,
 * H, and the first + vf_coeff x the second - ent_coeff x the third; the caller adds the workgroups (one sum over dim 0)
 * and divides by T rows.  No atomics, fixed summation order: two runs are bitwise equal.
 * Contract: exactly one launch, asynchronous on `stream`; no allocation, no workspace, no synchronisation; graph-
 * capturable from the first call; any T >= 1, rows >= 1, heads in 1 .. MAPF_VTRACE_MAX_HEADS.  Writes vs and pg_adv
 * [T][rows] and, unless NULL, logp [T][rows], dlogits [T][rows][heads][5], dvalues [T][rows] and partials; nothing else is
 * written, also when rows is not a multiple of the kernel's MAPF_VTRACE_TILE_ROWS-row tile, and nothing outside the inputs is
 * read.  t is walked from the end in chunks of MAPF_VTRACE_CHUNK steps, the recursion's state carried between them.
 * MAPF_ERR_CONFIG, and nothing is launched: T < 1, rows < 1, heads outside the range, a null input, vs or pg_adv, a non-
 * finite or negative scalar, gamma or lam above 1. */
#define MAPF_VTRACE_MAX_HEADS 64
#define MAPF_VTRACE_CHUNK 32
#define MAPF_VTRACE_TILE_ROWS 32
int mapf_vtrace_loss(int32_t T, int32_t rows, int32_t heads, const float *logits /* device [T][rows][heads][5] */,
                     const int8_t *actions /* device [T][rows][heads] */, const float *behaviour_logp, const float *values,
                     const float *rewards /* device [T][rows] */, const uint8_t *ended /* device [T][rows] */,
                     const float *bootstrap /* device [rows] */, float gamma, float lam, float clip_rho, float clip_c,
                     float clip_pg_rho, float vf_coeff, float ent_coeff, float *vs, float *pg_adv /* device [T][rows] */,
                     float *logp, float *dlogits, float *dvalues /* or NULL */, float *partials /* or NULL */, void *stream);
int32_t mapf_vtrace_partials(int32_t rows);

/* The PPO objective on a minibatch: clipped surrogate, clipped value error, entropy, the KL penalty against the behaviour
 * policy and their gradients with respect to the logits and the values, one launch (the network's forward and backward,
 * the advantages and the value targets are the caller's).  No handle.  Per element (t, row), with `heads` five-way action
 * heads (an agent row of the multi-agent env has one head; an env row of a joint fragment has N), everything in fp32:
 *   lp_k  = log_softmax(logits[t][row] of head k);      p = exp(lp)
 *   lq_k  = log_softmax(old_logits[t][row] of head k);  q = exp(lq)
 *   logp  = sum_k lp_k[a_k];   H = sum_k H_k,  H_k = -sum_j p_kj lp_kj;   KL = sum_k sum_j q_kj (lq_kj - lp_kj)
 *   ratio = exp(logp - old_logp);   A = adv
 *   s     = min(A ratio, A clamp(ratio, 1 - clip, 1 + clip))
 *   e     = (value - target)^2;     v = min(e, vf_clip)
 *   loss  = -s + vf_coeff v - ent_coeff H + kl_coeff[g] KL
 * A probability of exactly 0 adds 0 to H and to KL and has a 0 entropy gradient (never 0 x inf); a ratio that overflows to
 * +inf under a positive advantage clips to 1 + clip.  An action byte outside 0 .. 4 is clamped before it indexes anything.
 * Groups: row r belongs to policy g = r % groups (the interleaved agent rows b * N + a of one policy per agent, as the
 * grouped LSTM calls take them; rows is a multiple of groups).  Every mean is over the T rows / groups elements of one
 * group and the objective is the SUM over the groups of their means, so all gradients share the scale c = groups / (T rows):
 *   g_logp        = A ratio where A ratio <= A clamp(ratio, ..) (a tie included), else 0         (torch.minimum / clamp)
 *   dlogits[k][j] = c [ -g_logp (1[j = a_k] - p_kj) + ent_coeff p_kj (lp_kj + H_k) + kl_coeff[g] (p_kj - q_kj) ]
 *   dvalues       = c vf_coeff 2 (value - target) where e <= vf_clip, else 0
 * kl_coeff is a DEVICE pointer to `groups` floats, read by the kernel (as mapf_qnet_act reads epsilon): a captured graph
 * follows an adapted coefficient without recapture.  kl_coeff = NULL: no KL term, old_logits is not read and may be NULL,
 * kl (when given) is written as 0 and the KL column of the partials is 0.
 * Outputs, each may be NULL: logp, kl [T][rows], dlogits [T][rows][heads][5], dvalues [T][rows], and
 * partials [mapf_ppo_partials(rows, groups)][5]: per tile the sums over its (t, row) of -s, v, H, KL, and the first +
 * vf_coeff x the second - ent_coeff x the third + kl_coeff[g] x the fourth.  A tile is MAPF_PPO_TILE_ROWS rows OF ONE GROUP
 * and all T; tiles are ordered group-major, so view(groups, tiles per group, 5).sum(1) is the per-policy sums, which the
 * caller divides by T rows / groups.  mapf_ppo_partials(rows, groups) = groups * ceil(rows / groups / 32); 0 for rows <= 0,
 * groups < 1 or rows no multiple of groups.  No atomics, fixed summation order: two runs are bitwise equal.  What a tile
 * computes does not depend on groups: a group's outputs equal, bit for bit, the groups = 1 call on its rows alone.
 * Contract: exactly one launch, asynchronous on `stream`; no allocation, no workspace, no synchronisation; graph-
 * capturable from the first call; any T >= 1, rows >= 1, heads in 1 .. MAPF_PPO_MAX_HEADS.  Nothing but the non-NULL outputs
 * is written, also when a group's rows are no multiple of the tile, and nothing outside the inputs is read.  t is walked in
 * chunks of MAPF_PPO_CHUNK steps; nothing is carried between them, and no output depends on where a chunk begins.
 * MAPF_ERR_CONFIG, and nothing is launched: T < 1, rows < 1, heads outside the range, groups < 1, rows % groups != 0, a null
 * logits, actions, old_logp, adv, values or targets, a kl_coeff with a null old_logits, a non-finite or negative clip,
 * vf_clip, vf_coeff or ent_coeff, clip >= 1. */
#define MAPF_PPO_MAX_HEADS 64
#define MAPF_PPO_TILE_ROWS 32
#define MAPF_PPO_CHUNK 32
int mapf_ppo_loss(int32_t T, int32_t rows, int32_t heads, int32_t groups, const float *logits /* device [T][rows][heads][5] */,
                  const float *old_logits /* device [T][rows][heads][5], or NULL without kl_coeff */,
                  const int8_t *actions /* device [T][rows][heads] */, const float *old_logp, const float *adv,
                  const float *values, const float *targets /* device [T][rows] */, float clip, float vf_clip, float vf_coeff,
                  float ent_coeff, const float *kl_coeff /* device [groups] or NULL */, float *logp, float *kl, float *dlogits,
                  float *dvalues, float *partials /* each or NULL */, void *stream);
int32_t mapf_ppo_partials(int32_t rows, int32_t groups);

/* The same launch with per-group hyperparameters (a population of policies with one setting each in one minibatch):
 * mapf_ppo_loss's argument list plus hp, a DEVICE pointer to [groups][4] floats: clip, vf_clip, vf_coeff, ent_coeff of group
 * g, read by the workgroup where it reads kl_coeff[g], so the owner changes them between two launches without a
 * synchronisation and a captured graph follows them without recapture.  1 - clip and 1 + clip are formed from the group's
 * clip exactly as the host forms them from the scalar ((float)(1.0 - (double)clip)): group g's logp, kl, dlogits, dvalues
 * and partials equal, bit for bit, the groups = 1 scalar call on its rows with hp[g]'s values.  With hp the four scalars are
 * neither read nor checked.  The host cannot see hp: keeping every clip in [0, 1) and every value finite and >= 0 is the
 * caller's duty (learner.PPOLearner validates each value before it writes it).  hp = NULL: mapf_ppo_loss, bit for bit.  The
 * contract and the other refusals are mapf_ppo_loss's. */
int mapf_ppo_loss_hp(int32_t T, int32_t rows, int32_t heads, int32_t groups, const float *logits, const float *old_logits,
                     const int8_t *actions, const float *old_logp, const float *adv, const float *values, const float *targets,
                     float clip, float vf_clip, float vf_coeff, float ent_coeff, const float *kl_coeff /* device [groups] or NULL */,
                     const float *hp /* device [groups][4]: clip, vf_clip, vf_coeff, ent_coeff; NULL: the scalars */, float *logp,
                     float *kl, float *dlogits, float *dvalues, float *partials /* each or NULL */, void *stream);

/* The behaviour-cloning objective on a minibatch: the negative log-likelihood of an expert's actions under the policy's
 * logits, an optional regression of the value head, an optional entropy bonus, the count of heads whose greedy action is the
 * expert's, and the gradients with respect to the logits and the values, one launch (the network's forward and backward and
 * the value targets are the caller's).  No handle.  Per element (t, row), with `heads` five-way action heads (as in
 * mapf_ppo_loss), everything in fp32:
 *   lp_k  = log_softmax(logits[t][row] of head k);  p = exp(lp)
 *   e_k   = expert[t][row][k], clamped to 0 .. 4 before it indexes anything
 *   nll   = -sum_k lp_k[e_k]
 *   H     = sum_k H_k,  H_k = -sum_j p_kj lp_kj
 *   hits  = the number of heads k with argmax_j logits_kj (the lowest j on ties) == e_k
 *   v     = 0.5 (value - target)^2      (only with values and targets: both or neither; without them v = 0)
 *   loss  = nll + vf_coeff v - ent_coeff H
 * A probability of exactly 0 adds 0 to H and has a 0 entropy gradient (never 0 x inf).  The argmax compares the fp32 logits
 * as they are read, with no arithmetic.
 * Groups: row r belongs to policy g = r % groups, exactly as in mapf_ppo_loss; rows is a multiple of groups.  Every mean is
 * over the T rows / groups elements of one group and the objective is the SUM over the groups of their means, so all
 * gradients share the scale c = groups / (T rows):
 *   dlogits[k][j] = c [ (p_kj - 1[j = e_k]) + ent_coeff p_kj (lp_kj + H_k) ]
 *   dvalues       = c vf_coeff (value - target)
 * Outputs, each may be NULL: nll [T][rows], dlogits [T][rows][heads][5], dvalues [T][rows] (needs values and targets), and
 * partials [mapf_bc_partials(rows, groups)][5]: per tile the sums over its (t, row) of nll, v, H, hits, and the first +
 * vf_coeff x the second - ent_coeff x the third.  A tile is MAPF_BC_TILE_ROWS rows OF ONE GROUP and all T; tiles are ordered
 * group-major, so view(groups, tiles per group, 5).sum(1) is the per-policy sums, which the caller divides by T rows /
 * groups (the hits by heads as well, for the accuracy).  The hit count of a tile is a sum of small integers in fp32: it is
 * exact while T * MAPF_BC_TILE_ROWS * heads < 2^24.  mapf_bc_partials(rows, groups) = groups * ceil(rows / groups / 32); 0
 * for rows <= 0, groups < 1 or rows no multiple of groups.  No atomics, fixed summation order: two runs are bitwise equal.
 * What a tile computes does not depend on groups: a group's outputs equal, bit for bit, the groups = 1 call on its rows
 * alone.
 * Contract: exactly one launch, asynchronous on `stream`; no allocation, no workspace, no synchronisation; graph-
 * capturable from the first call; any T >= 1, rows >= 1, heads in 1 .. MAPF_BC_MAX_HEADS.  Nothing but the non-NULL outputs
 * is written, also when a group's rows are no multiple of the tile, and nothing outside the inputs is read.  t is walked in
 * chunks of MAPF_BC_CHUNK steps; nothing is carried between them, and no output depends on where a chunk begins.
 * MAPF_ERR_CONFIG, and nothing is launched: T < 1, rows < 1, heads outside the range, groups < 1, rows % groups != 0, a null
 * logits or expert, only one of values and targets, a dvalues without them, a non-finite or negative vf_coeff or
 * ent_coeff. */
#define MAPF_BC_MAX_HEADS 64
#define MAPF_BC_TILE_ROWS 32
#define MAPF_BC_CHUNK 32
int mapf_bc_loss(int32_t T, int32_t rows, int32_t heads, int32_t groups, const float *logits /* device [T][rows][heads][5] */,
                 const int8_t *expert /* device [T][rows][heads] */, const float *values,
                 const float *targets /* device [T][rows], both or neither */, float vf_coeff, float ent_coeff, float *nll,
                 float *dlogits, float *dvalues, float *partials /* each or NULL */, void *stream);
int32_t mapf_bc_partials(int32_t rows, int32_t groups);

/* DQN: the Q-network's act, prioritised sampling from a replay ring and the TD objective (the reference's ALGO_NAME = "DQN",
 * src/agents/dqn.py: a 32-32 feed-forward net behind RLlib's default module -- the whole observation is the feature vector,
 * mask floats included -- with RLlib's documented defaults: dueling heads, double-Q, Huber loss, n-step 1, hard target
 * updates, epsilon-greedy exploration, a prioritised buffer with alpha 0.6 and beta 0.4).
 *
 * Q-network.  A handle is independent of an env handle and works on `rows` agent rows.  Config: obs_len = L in [1, 130];
 * hidden = MAPF_QNET_HIDDEN = 32 (any other width is MAPF_ERR_CONFIG); device.  Per row, everything in fp32:
 *   a1  = tanh(W1 obs + b1)               W1 [32][L]
 *   a2  = tanh(W2 a1 + b2)                W2 [32][32]
 *   adv = Wa a2 + ba  (5 values);   val = Wv a2 + bv
 *   q_j = val + adv_j - mean(adv)
 *   greedy action = argmax_j q_j, lowest j on ties
 * Exploration (epsilon != NULL; `mix` is the splitmix64 finalizer of the fused recurrent policy above):
 *   x = mix(seed ^ ((uint64)row << 32 | draws[row]));   u = ((x >> 40) + 0.5) * 2^-24
 *   the row explores iff u < eps (compared in double), and then takes action (mix(x + 0x9E3779B97F4A7C15) >> 40) % 5
 * eps is read from DEVICE memory (epsilon points to one float), so a captured graph follows a schedule without recapture.
 * epsilon = NULL means greedy, and draws is neither read nor written; otherwise draws[row] (uint32) is read and stored plus
 * one, unless mode has MAPF_QNET_PEEK.  Precision as for the policy: fp32 operands, fp32 accumulation on
 * v_mfma_f32_32x32x2_f32, any summation order; no reduced precision.
 * Parameters: the flat fp32 vector in the state_dict order of dqn.QNetwork:
 *   fc1.weight [32][L], fc1.bias, fc2.weight [32][32], fc2.bias, adv.weight [5][32], adv.bias, val.weight [1][32], val.bias
 * mapf_qnet_param_count returns its length (0 for a null handle); mapf_qnet_set_params is one asynchronous repacking launch
 * on `stream` (MAPF_ERR_CONFIG for a null argument or another count).
 * Outputs: action int8 [rows]; q float [rows][5] or NULL.
 * Contract: exactly one launch, asynchronous on `stream`; no allocation, no workspace, no synchronisation; graph-capturable
 * from the first call of a process; two handles may be in flight at once.  It writes the `rows` elements of each non-NULL
 * output and, when exploring without PEEK, of draws, and nothing else, also when rows is not a multiple of the kernel's
 * 32-row tile.  It never reads outside obs[rows][L], draws[rows] or epsilon[0]; the zero-padded K tail of the first product
 * is not fed from memory.  MAPF_ERR_CONFIG: a null handle, obs or action, null draws with a non-null epsilon, rows < 1,
 * unknown mode bits.  MAPF_ERR_STATE: before mapf_qnet_set_params.  Nothing is launched in either case. */
#define MAPF_QNET_HIDDEN 32
#define MAPF_QNET_PEEK 2 /* = MAPF_POLICY_PEEK */
typedef struct mapf_qnet_config {
    int32_t obs_len; /* L */
    int32_t hidden;  /* MAPF_QNET_HIDDEN */
    int32_t device;
} mapf_qnet_config;
typedef struct mapf_qnet *mapf_qnet_handle;
int mapf_qnet_create(const mapf_qnet_config *cfg /* host */, mapf_qnet_handle *out);
int mapf_qnet_destroy(mapf_qnet_handle h);
int64_t mapf_qnet_param_count(mapf_qnet_handle h);
int mapf_qnet_set_params(mapf_qnet_handle h, const float *params /* device, flat */, int64_t count, void *stream);
int mapf_qnet_act(mapf_qnet_handle h, int32_t rows, const float *obs /* device [rows][L] */,
                  const float *epsilon /* device [1] or NULL: greedy */, uint32_t *draws /* device [rows], in/out */,
                  uint64_t seed, int32_t mode, int8_t *action /* device [rows] */, float *q /* device [rows][5] or NULL */,
                  void *stream);

/* Replay ring (dqn.ReplayBuffer keeps it; stated here because the sampler and the objective work on its weights): S time
 * slots of R rows; transition (g, row) is (obs[g], action[g], reward[g], ended[g], obs[(g + 1) mod S]).  Its weight is a
 * uint32, non-zero exactly while both observations are in the ring; ended = terminated | truncated.  A priority is
 *   w = clamp(rint((|td| + 1e-6)^alpha * 2^16), 1, 2^20)
 * so that sampling is exact in integers: with count = S R <= MAPF_REPLAY_MAX_COUNT = 2^26 weights and
 * K <= MAPF_REPLAY_MAX_SAMPLES = 65536 samples every total and every k W stays below 2^62.
 *
 * mapf_replay_sample: stratified prioritised sampling.  W = sum of weights (exact, 64 bits), n_valid = the number of non-zero
 * weights.  For k = 0 .. K - 1:
 *   lo = floor(k W / K);  hi = floor((k + 1) W / K)
 *   x_k = mix(seed ^ ((uint64)draws[0] << 32 | k));   target = lo + x_k mod max(hi - lo, 1)
 *   idx[k] = the smallest flat index i with sum_{j <= i} w_j > target;   wk[k] = weights[idx[k]]
 * stats = (W, n_valid) as int64; draws[0] (uint32, device) is stored plus one.  When W = 0 every idx[k] is -1 and every wk[k]
 * is 0.  Integer arithmetic: the result does not depend on the order of summation and equals a cumulative sum in uint64
 * followed by an upper-bound search, element for element.
 * Contract: exactly three launches on `stream` (sums of chunks of MAPF_REPLAY_CHUNK weights; one workgroup that turns them
 * into an inclusive prefix and takes the draw counter; a search per sample), no atomics, no allocation, no synchronisation,
 * graph-capturable from the first call.  workspace: mapf_replay_sample_workspace_bytes(count) bytes (0 for a count out of
 * range), 8-byte aligned, device; nothing outside it, idx[K], wk[K], stats[2] and draws[0] is written and nothing outside
 * weights[count] is read.  wk and stats may be NULL.  MAPF_ERR_CONFIG, and nothing is launched: a null weights, draws,
 * workspace or idx, a misaligned workspace, count or K out of range. */
#define MAPF_REPLAY_MAX_COUNT (1 << 26)
#define MAPF_REPLAY_MAX_SAMPLES 65536
#define MAPF_REPLAY_CHUNK 256
int64_t mapf_replay_sample_workspace_bytes(int64_t count);
int mapf_replay_sample(const uint32_t *weights /* device [count] */, int64_t count, int32_t K, uint32_t *draws /* device [1] */,
                       uint64_t seed, void *workspace, int32_t *idx /* device [K] */, uint32_t *wk /* device [K] or NULL */,
                       int64_t *stats /* device [2] or NULL */, void *stream);

/* mapf_dqn_td_loss: the double-Q Huber objective on K sampled transitions, its gradient with respect to q and the new
 * priorities, one launch (the network's forward and backward are the caller's).  Per sample, in fp32:
 *   a   = action clamped to 0 .. 4 (as in mapf_vtrace_loss)
 *   a*  = argmax_j qn_online_j, lowest j on ties       (qn_online = qn_target gives plain DQN)
 *   y   = ended ? reward : reward + gamma * qn_target[a*]
 *   td  = q[a] - y
 *   l   = |td| <= delta ? 0.5 td^2 : delta (|td| - 0.5 delta)
 *   loss = mean(isw * l);   dq[k][j] = isw_k * clamp(td_k, -delta, delta) / K at j = a_k, 0 elsewhere
 *   new_w[k] = the priority rule above, evaluated in double from the fp32 q[a], reward, gamma and qn_target[a*]
 * y of an ended step is the short form, never a multiplication by 0: the next observation of an ended step belongs to the next
 * episode, qn_online and qn_target of that sample are not read, and nothing of them can leak, a NaN included.
 * With idx and weights (both or neither; weights has `count` elements), weights[idx[k]] = new_w[k] for every idx[k] in
 * 0 .. count - 1; duplicates of an index are expected to carry equal inputs and therefore bitwise equal values.
 * Outputs, each may be NULL: td [K], dq [K][5], new_w uint32 [K], partials [mapf_dqn_td_partials(K)][2] = per workgroup of
 * MAPF_DQN_TD_TILE samples the sums of isw * l and of |td|; the caller adds the workgroups and divides by K.  No atomics,
 * fixed summation order: two runs are bitwise equal.
 * Contract: exactly one launch, asynchronous on `stream`; no allocation, no workspace, no synchronisation; graph-capturable
 * from the first call; nothing but the outputs named is written and nothing outside the inputs is read.  MAPF_ERR_CONFIG,
 * and nothing is launched: K < 1 or above MAPF_REPLAY_MAX_SAMPLES, a null input, only one of idx and weights, count out of
 * range, gamma or alpha outside [0, 1], delta not positive, a non-finite scalar. */
#define MAPF_DQN_TD_TILE 256
int mapf_dqn_td_loss(int32_t K, const float *q, const float *qn_online, const float *qn_target /* device [K][5] */,
                     const int8_t *action, const float *reward, const uint8_t *ended, const float *isw /* device [K] */,
                     float gamma, float delta, float alpha, const int32_t *idx /* device [K] or NULL */,
                     uint32_t *weights /* device [count] or NULL */, int64_t count, float *td, float *dq, uint32_t *new_w,
                     float *partials, void *stream);
int32_t mapf_dqn_td_partials(int32_t K);

#ifdef __cplusplus
}
#endif
#endif
