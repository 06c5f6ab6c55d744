/*
 * okenv.h -- C ABI of the MI355X-native batched Environment step (libokenv.so).
 *
 * This is the drop-in boundary for the hot path of goksanisil23/OpenKitchen (paths below are relative to
 * the reference tree): everything `Environment::step()` does per step -- Agent kinematics, the
 * standstill timeout, the 2-D raycast lidar against the RaceTrack's boundary segments and the
 * lidar-based crash test -- for N agents x R rays per launch, with the agent state resident on the GPU
 * as struct-of-arrays.  The C++ classes in include/Environment/ (same names and members as the
 * reference's) are thin hosts over these entry points; INTEGRATION.md shows the binding a maintainer of
 * the reference would add.
 *
 * Conventions: every function returns an int status (OKENV_OK == 0, negative on error) unless noted; no
 * exception crosses this boundary; `okenv_last_error` returns a message for the most recent failure on
 * the handle (or globally, for NULL).  Host buffers are caller-owned; device buffers are library-owned.
 * A handle owns one HIP stream; work is enqueued asynchronously and the `get`/`download` calls
 * synchronise.  A handle is used by one thread at a time; multi-GPU means one handle per device (one
 * process per GPU in bench.py).  Pointers passed to `okenv_set_field` / `okenv_get_field` /
 * `okenv_set_actions` may be host OR device pointers (hipMemcpyDefault).
 */
#ifndef OKENV_H
#define OKENV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define OKENV_API
#else
#define OKENV_API __attribute__((visibility("default")))
#endif

#define OKENV_OK 0
#define OKENV_ERR_INVALID (-1)  /* bad argument */
#define OKENV_ERR_HIP (-2)      /* a HIP runtime call failed */
#define OKENV_ERR_NO_DEVICE (-3)/* no usable GPU: the product path has NO CPU fallback */
#define OKENV_ERR_IO (-4)       /* track CSV could not be read */
#define OKENV_ERR_STATE (-5)    /* call not valid in the handle's current state */

typedef struct okenv *okenv_t;
typedef struct okenv_track *okenv_track_t;

/* Agent::MovementMode, Environment/Agent.h:20-25 */
#define OKENV_MODE_VELOCITY 0
#define OKENV_MODE_ACCELERATION 1
#define OKENV_MODE_MANUAL 2

/* okenv_create flags */
#define OKENV_FLAG_NONE 0u
#define OKENV_FLAG_FORCE_GLOBAL_GRID 1u /* keep the grid in global memory even if it fits LDS (testing) */
#define OKENV_FLAG_BRUTE_FORCE 2u       /* sweep all segments like the reference kernel (testing / ablation) */

/*
 * State fields (struct-of-arrays).  One value per agent unless marked [N*R] (agent-major, ray-minor).
 * They mirror, field for field, what the reference keeps per Agent (Environment/Agent.h:56-81), per
 * DisplacementStats (Environment/Environment.h:17-27) and per Ray_ (Environment/Typedefs.h:91-99).
 */
enum okenv_field {
    OKENV_F_POS_X = 0,     /* f32  Agent::pos_.x                                    */
    OKENV_F_POS_Y = 1,     /* f32  Agent::pos_.y                                    */
    OKENV_F_ROT = 2,       /* f32  Agent::rot_ [deg], never wrapped                 */
    OKENV_F_SPEED = 3,     /* f32  Agent::speed_                                    */
    OKENV_F_ACC = 4,       /* f32  Agent::acceleration_                             */
    OKENV_F_THROTTLE = 5,  /* f32  Agent::current_action_.throttle_delta            */
    OKENV_F_STEER = 6,     /* f32  Agent::current_action_.steering_delta            */
    OKENV_F_MODE = 7,      /* u8   Agent::movement_mode_                            */
    OKENV_F_CRASHED = 8,   /* u8   Agent::crashed_                                  */
    OKENV_F_TIMED_OUT = 9, /* u8   Agent::timed_out_                                */
    OKENV_F_DISP_CTR = 10, /* u32  DisplacementStats::displacement_ctr              */
    OKENV_F_DISP_X = 11,   /* f32  DisplacementStats::init_pos.x                    */
    OKENV_F_DISP_Y = 12,   /* f32  DisplacementStats::init_pos.y                    */
    OKENV_F_DISP_TO = 13,  /* u8   DisplacementStats::displacement_timed_out        */
    OKENV_F_HIT_X = 14,    /* f32 [N*R] Ray_::hit_x (world frame, persists while crashed) */
    OKENV_F_HIT_Y = 15,    /* f32 [N*R] Ray_::hit_y                                 */
    OKENV_F_REL_X = 16,    /* f32 [N*R] Agent::sensor_hits_[r].x ("robot frame")    */
    OKENV_F_REL_Y = 17,    /* f32 [N*R] Agent::sensor_hits_[r].y                    */
    OKENV_F_DIST = 18,     /* f32 [N*R] Agent::sensor_hits_[r].norm()               */
    OKENV_F_COUNT = 19,
    /* rollout bookkeeping; exist after okenv_tracker_create (not part of okenv_state_view / snapshots) */
    OKENV_F_REWARD = 19,         /* f32  reward of the last okenv_tracker_update              */
    OKENV_F_FITNESS = 20,        /* f32  CmaEsAgent::fitness_ / return of the running episode  */
    OKENV_F_TRACK_IDX = 21,      /* i32  prev_track_idx_ (main_eigen.cpp:84); PROGRESS reward only, else 0 */
    OKENV_F_EPISODE_STEPS = 22,  /* u32  updates since the episode began                      */
    OKENV_F_EPISODE_RETURN = 23, /* f32  fitness at the end of the last finished episode     */
    OKENV_F_PREV_CRASHED = 24,   /* u8   crashed_ as the last okenv_tracker_update / _begin saw it (detects re-placed agents) */
    OKENV_F_COUNT_ALL = 25
};

/* Struct-of-pointers form of the per-agent state, for one-call upload/download by the C++ facade.
 * NULL members are skipped. */
typedef struct okenv_state_view {
    float *pos_x, *pos_y, *rot, *speed, *acc, *throttle, *steer;
    uint8_t *mode, *crashed, *timed_out;
    uint32_t *disp_ctr;
    float *disp_x, *disp_y;
    uint8_t *disp_timed_out;
} okenv_state_view;

typedef struct okenv_info {
    int32_t num_agents, num_rays, num_segments;
    int32_t grid_nx, grid_ny;
    float grid_cell;
    int32_t grid_refs;        /* total segment registrations */
    int32_t grid_in_lds;      /* 1: grid + segments staged in LDS per workgroup, 0: read from global memory */
    int32_t lds_bytes;        /* dynamic LDS per workgroup */
    int32_t block_threads;    /* workgroup size of the step kernel */
    int32_t grid_blocks;      /* workgroups per launch */
    int32_t lanes_per_agent;  /* G: power of two >= R, capped at 64 */
    int32_t device;
    int32_t agents_per_block; /* > 0: tiny population, that many agents per workgroup (the other lanes only stage)   */
    int32_t packed_resident;  /* 1: a resident step kernel is serving okenv_step_packed right now                    */
    int32_t packed_resident_steps; /* okenv_step_packed calls served by a resident kernel so far                     */
    int32_t packed_fallbacks; /* ... of which the resident kernel had left: redone by a launch of their own          */
    int32_t compute_units;    /* CUs of the device as HIP reports them (256 on an MI355X in SPX mode): what the launch geometry,  */
                              /* the lane-group rule for small populations and the tail-kernel hand-over point are sized by     */
    int32_t front_back_bytes; /* > 0: the segment set is split (ok_grid.h): bytes of the [front | back] images the cooperative     */
                              /* kernel stages instead of the combined image; 0: no split (not a track, or OKENV_FRONT_BACK=0)     */
    int32_t back_segments;    /* segments in the back image: looked at only by rays whose origin is not certified / ambiguous walks */
} okenv_info;

/* ---- lifetime ------------------------------------------------------------------------------------ */

/*
 * Replaces: TrackSegments::uploadToDevice (Environment/TrackSegments.cu:69-76) + CollisionChecker::Impl
 * constructor (Environment/CollisionChecker.cu:76-86) + Environment's displacement_stats_.resize
 * (Environment/Environment.cpp:61).  `segments_xyxy` is the reference's Segment2d[S] layout
 * (x1,y1,x2,y2); `ray_angles_deg` is Agent::sensor_ray_angles_ (all agents share one fan,
 * CollisionChecker.cu:82).  All state starts zeroed (mode VELOCITY, not crashed).
 * `grid_cell` <= 0 selects the default cell edge.
 * A segment set in TrackSegments order whose boundary polylines close (every track the reference builds) is additionally split
 * into the segments a ray from between the inner boundaries can hit first and the rest (the outer polylines, 3 px behind the
 * inner ones): the step kernels look at the rest only for rays whose origin is not certified to lie between the inner boundaries
 * -- same first hit, bit for bit, about half the points per ray (okenv_info.front_back_bytes / back_segments,
 * okenv_work_stats_split; environment variable OKENV_FRONT_BACK=0 switches it off).  Any other segment set is stepped as before.
 */
OKENV_API int okenv_create(okenv_t *out, const float *segments_xyxy, int32_t num_segments, int32_t num_agents,
                           int32_t num_rays, const float *ray_angles_deg, int32_t device, uint32_t flags,
                           float grid_cell);
/* Replaces ~CollisionChecker / ~TrackSegments (Environment/CollisionChecker.cu:88-94, TrackSegments.cu:44-51). */
OKENV_API int okenv_destroy(okenv_t h);
OKENV_API int okenv_get_info(okenv_t h, okenv_info *out);
/* Message for the last failure on `h` (or the last create failure if h is NULL).  Never NULL. */
OKENV_API const char *okenv_last_error(okenv_t h);
/* Agent::sensor_offset_ (Environment/Agent.h:61), shared by all agents; default 0. */
OKENV_API int okenv_set_sensor_offset(okenv_t h, float offset);
/* Centre line + headings (RaceTrack::track_data_points_.x_m/y_m, headings_), needed by the nearest-index
 * query and by the on-device reset in okenv_rollout_random. */
OKENV_API int okenv_set_centerline(okenv_t h, const float *x, const float *y, const float *heading_deg, int32_t num_points);
/* Use an externally owned hipStream_t (e.g. torch's current stream, or a stream being captured into a hipGraph)
 * instead of the private one.  Does not synchronise: ordering against work already queued is the caller's. */
OKENV_API int okenv_set_stream(okenv_t h, void *hip_stream);
OKENV_API int okenv_sync(okenv_t h);

/* ---- state access -------------------------------------------------------------------------------- */

OKENV_API int okenv_set_field(okenv_t h, int32_t field, const void *src);
OKENV_API int okenv_get_field(okenv_t h, int32_t field, void *dst); /* synchronises */
OKENV_API int okenv_upload_state(okenv_t h, const okenv_state_view *host_view);
OKENV_API int okenv_download_state(okenv_t h, const okenv_state_view *host_view); /* synchronises */
/* Agent::current_action_ for every agent (what callers write before Environment::step, Template/main.cpp:107-110). */
OKENV_API int okenv_set_actions(okenv_t h, const float *throttle, const float *steer);
/* Agent::reset (Environment/Agent.cpp:123-135) for agents idx[0..n): pose set, speed/acc/action zeroed,
 * crashed/timed_out cleared; DisplacementStats untouched, as in the reference.  Host arrays. */
OKENV_API int okenv_reset_agents(okenv_t h, const int32_t *idx, const float *x, const float *y, const float *rot_deg, int32_t n);
/* ---- device-side Environment::resetAgent ----------------------------- */

/* the booleans of Environment::resetAgent(agent, pick_random_point, randomize_lane, randomize_heading)
 * (Environment/Environment.h:47-50); values shared with include/okenv_math.h (OK_RESET_*) */
#define OKENV_RESET_RANDOM_POINT 1u
#define OKENV_RESET_RANDOM_LANE 2u
#define OKENV_RESET_RANDOM_HEADING 4u
#define OKENV_RESET_ONLY_DONE 8u /* batch call only: skip agents whose crashed_ flag is clear */

/* RaceTrack::left_bound_inner_ / right_bound_inner_ (Environment/RaceTrack.h:77) as xy pairs, what the lane
 * randomisation interpolates between (Environment/Environment.cpp:108-113).  Host or device pointers. */
OKENV_API int okenv_set_lane_bounds(okenv_t h, const float *left_inner_xy, const float *right_inner_xy, int32_t num_points);
/* Environment::resetAgent (Environment/Environment.cpp:79-122) for agents idx[0..n) (idx NULL: all agents, n ignored),
 * on the device.  raylib's GetRandomValue is replaced by Philox4x32 keyed (seed; agent_base + agent, epoch), see
 * ok_draw_reset in okenv_math.h; entry j of the call takes the reference's static call counter as epoch + j, so a loop
 * `for (agent : agents) env.resetAgent(agent, ...)` is one call.  idx may be a host or a device pointer.
 * Without OKENV_RESET_RANDOM_POINT every agent goes to RaceTrack::kStartingIdx with the track heading. */
OKENV_API int okenv_reset_random(okenv_t h, const int32_t *idx, int32_t n, uint32_t flags, uint32_t seed, uint32_t epoch,
                                 uint32_t agent_base);
/* Per-agent auto-reset for continuous training: while enabled, okenv_step and okenv_rollout_policy begin every step
 * by applying resetAgent(flags) to the agents whose crashed_ flag is set, drawing from Philox (seed; agent_base +
 * agent, step count) with call-counter parity agent + step count; that step then runs with the zeroed action, i.e.
 * it is the "initial observation" step callers take after a reset (RLRacers/PPO/ppo_sim.cpp:53-60).  The flags
 * of the crash stay readable until that next step. */
OKENV_API int okenv_set_auto_reset(okenv_t h, int32_t enabled, uint32_t flags, uint32_t seed, uint32_t agent_base);
/* Environment steps taken so far by okenv_step / okenv_rollout_policy on this handle (the auto-reset epoch).  While
 * auto-reset is on the count lives on the device and is advanced on the stream behind every step, so a captured
 * hipGraph of step launches replays with advancing epochs; reading it then synchronises. */
OKENV_API int okenv_get_step_count(okenv_t h, uint32_t *out);
OKENV_API int okenv_set_step_count(okenv_t h, uint32_t value);

/* ---- rollout bookkeeping of the current-API population callers -------- */

/* The per-step loop the living callers run after env.step() (CovarianceMatrixAdaptationEvolution/main_eigen.cpp:
 * 143-158, RLRacers/PPO/ppo_sim.cpp:73-88), for all agents on the device. */
#define OKENV_REWARD_STEP 0     /* +1 per step for every agent, crashed or not (ppo_sim.cpp:77-80)                   */
#define OKENV_REWARD_PROGRESS 1 /* |curr - prev nearest centre-line index| while alive, fitness := 0 once timed out  */
                                /* (main_eigen.cpp:147-158; the index difference is NOT wrapped at the lap seam)     */
OKENV_API int okenv_tracker_create(okenv_t h, int32_t reward_kind);
/* Start of an episode for every agent: prev_track_idx_ = findNearestTrackIndexBruteForce(pos_), fitness_ = 0
 * (main_eigen.cpp:128-133, CmaEsAgent::reset :70-74).  Call after the initial-observation step. */
OKENV_API int okenv_tracker_begin(okenv_t h);
/* The bookkeeping after one Environment::step.  An agent that was crashed at the previous update and is not now has
 * been re-placed (okenv_reset_random or auto-reset): its episode restarts here with reward 0 (that step was its
 * initial observation).  An agent that crashes in this step gets OKENV_F_EPISODE_RETURN := fitness. */
OKENV_API int okenv_tracker_update(okenv_t h);

/* The CMA-ES candidates' controllers on the device (CovarianceMatrixAdaptationEvolution/Controller.cpp:3-23: fc1 rays ->
 * hidden, fc2 hidden -> hidden / 2, fc3 hidden / 2 -> 2, tanh after each; main_eigen.cpp:18-19 uses hidden = 16), one
 * parameter vector per agent in the order of torch's parameters() (Controller.cpp:36-53).  hidden: even, 2..64. */
OKENV_API int okenv_controller_create(okenv_t h, int32_t hidden);
OKENV_API int okenv_controller_num_params(okenv_t h, int32_t *out);
/* Controller::set_params for every agent: params[num_agents][num_params], host or device pointer (e.g. the solver's
 * sample tensor). */
OKENV_API int okenv_controller_set_params(okenv_t h, const float *params);
/* CmaEsAgent::updateAction for every agent (main_eigen.cpp:58-68): input ||sensor_hits_[i]|| / kSensorRange of the last
 * step, throttle_delta = throttle, steering_delta = output[0] * steering_scale (100 and 5 in the reference).  One kernel on
 * the handle's stream, no synchronisation: it can be captured into a HIP graph next to okenv_step. */
OKENV_API int okenv_controller_act(okenv_t h, float throttle, float steering_scale);
/* The inner loop of the CMA-ES racers (main_eigen.cpp:135-160), n_steps iterations in ONE launch: for every agent
 * { CmaEsAgent::updateAction (= okenv_controller_act); Environment::step; the fitness bookkeeping (= okenv_tracker_update) } with
 * the controller, the step and the bookkeeping fused into the step kernel -- same results, bit for bit, as the three calls made
 * n_steps times.  Needs okenv_controller_create, okenv_tracker_create (either reward kind) and the centre line.  Inside an
 * episode (okenv_episode_begin / _compact / _end, below) later launches cover only the agents that can still change and
 * okenv_episode_end returns the loop's own length, as for okenv_rollout_policy; episodes need OKENV_REWARD_PROGRESS (the +1
 * reward keeps counting for crashed agents, which an episode no longer steps).  hidden <= 4 x the handle's lanes per agent. */
OKENV_API int okenv_rollout_controller(okenv_t h, int32_t n_steps, float throttle, float steering_scale);

/* ---- expert drivers: FieldNavigators/ on the device -------------------
 * PotFieldAgent::updateAction (FieldNavigators/PotentialFieldAgent.hpp:52-84) with DataCollectorAgent's steering clamp
 * (FieldNavigators/collect_data/collect_data_random.cpp:59-65), or VFHAgent::updateAction (FieldNavigators/VFHAgent.hpp:53-123), for
 * every agent, towards the goal point of their callers: nearest centre-line index of the agent's position + lookahead, wrapped
 * modulo P (FieldNavigators/main.cpp:20-25) or clamped to P - 1 (collect_data_random.cpp:108-120).  The rule is restated in
 * include/okenv_math.h (ok_potfield_action, ok_vfh_action; the two spots where the reference is undefined are written there). */
#define OKENV_EXPERT_POTFIELD 0
#define OKENV_EXPERT_VFH 1

typedef struct okenv_expert_params {
    int32_t kind;          /* OKENV_EXPERT_POTFIELD | OKENV_EXPERT_VFH                                                    */
    int32_t lookahead;     /* kLookAheadIdx (PotentialFieldAgent.hpp:22, VFHAgent.hpp:21: 2), >= 0                        */
    int32_t goal_wrap;     /* != 0: (nearest + lookahead) % P (main.cpp:23); 0: min(nearest + lookahead, P - 1)           */
    float   k_att;         /* kAttractiveConstant  (PotentialFieldAgent.hpp:23: 100)                                      */
    float   k_rep;         /* kRepulsiveConstant   (:24: 10)                                                              */
    float   effect_range;  /* kObstacleEffectRange (:25: 5)                                                               */
    float   clamp_deg;     /* kSteeringAngleClampDeg (collect_data_random.cpp:45: 10); <= 0: no clamp (PotFieldAgent)     */
    float   vfh_throttle;  /* VFHAgent.hpp:120: 100                                                                       */
    int32_t vfh_threshold; /* kObstacleDistThreshold (VFHAgent.hpp:20: 1): a sector is occupied when count > threshold    */
} okenv_expert_params;

/* Where okenv_expert_act leaves this step's sample, besides the action fields: device pointers of the handle's device, each may
 * be NULL (skipped).  The observation is the one the action was computed from (what saveMeasurement writes,
 * collect_data_random.cpp:67-100). */
typedef struct okenv_expert_record {
    float   *action; /* [N][2]    throttle_delta, steering_delta                      */
    float   *dist;   /* [N][R]    OKENV_F_DIST                                         */
    float   *rel_xy; /* [N][R][2] OKENV_F_REL_X, OKENV_F_REL_Y interleaved             */
    uint8_t *alive;  /* [N]       !crashed_                                           */
} okenv_expert_record;

/* Attaches an expert to the handle (replaces an earlier one): validates, computes the per-ray cos / sin table in fp64 on the host
 * and uploads it.  Any fan for the potential field; 2 <= R <= 64 for VFH (num_sectors_ = R, fov_ = |last - first|).
 * OKENV_ERR_STATE without okenv_set_centerline; OKENV_ERR_INVALID for a NULL params pointer, an unknown kind, lookahead < 0 or
 * a VFH fan outside 2 .. 64 rays.  Synchronises. */
OKENV_API int okenv_expert_create(okenv_t h, const okenv_expert_params *params);
/* updateAction for every agent, crashed ones included (FieldNavigators/main.cpp:78-84 asks every agent): reads pos_, rot_ and the
 * last step's distances, writes OKENV_F_THROTTLE / OKENV_F_STEER and, when `rec` is given, the record slots.  One kernel on the
 * handle's stream, no synchronisation, no allocation: it can be captured into a HIP graph next to okenv_step (the contract of
 * okenv_controller_act; like it, it ends a running episode without the end-of-episode corrections).  OKENV_ERR_STATE before
 * okenv_expert_create or without a centre line. */
OKENV_API int okenv_expert_act(okenv_t h, const okenv_expert_record *rec);
/* The same rule on host arrays, no GPU needed: n agents, ray fan [num_rays], dist [n][num_rays]; the goal points come from the
 * centre line (cx, cy [num_points]) as above or, when goal_x / goal_y are not NULL, are given (cx / cy may then be NULL). */
OKENV_API int okenv_expert_act_host(const okenv_expert_params *params, const float *ray_angles_deg, int32_t num_rays, const float *cx,
                                    const float *cy, int32_t num_points, int32_t n, const float *pos_x, const float *pos_y, const float *rot_deg,
                                    const float *dist, const float *goal_x, const float *goal_y, float *throttle, float *steer);

/* ---- shared-network actors: RLRacers' PPO, REINFORCE and Deep-Q agents on the device (DESIGN.md
 * section 14) ----------------------------------------------------------------------------------------------------------------
 * updateAction of the agents that share ONE network (RLRacers/PPO/PPOAgent.hpp:68-102, Reinforce/Policy.hpp:22-29,
 * Deep_Q_Learning/DQAgent.hpp:85-104) for every agent of the handle: x = dist / kSensorRange, a policy network R -> H -> A and an
 * optional value network R -> Hv -> 1 (ReLU after the hidden layer), softmax + clamp + categorical sampling, arg-max, or
 * epsilon-greedy, and the action table from index to (throttle_delta, steering_delta).  The rule, with its summation order, its
 * exp and its Philox stream, is written out in include/okenv_math.h (ok_actor_*). */
#define OKENV_ACTOR_SAMPLE 0     /* PPO, REINFORCE: one categorical draw from the clamped softmax */
#define OKENV_ACTOR_GREEDY 1     /* evaluation: arg-max of the logits                             */
#define OKENV_ACTOR_EPS_GREEDY 2 /* Deep-Q: a uniform action with probability epsilon, else arg-max */

typedef struct okenv_actor_params {
    int32_t  hidden;             /* H, 1 .. 256                                                     */
    int32_t  num_actions;        /* A, 2 .. 8                                                       */
    int32_t  value_hidden;       /* Hv, 0 .. 256; 0: no value network                               */
    int32_t  mode;               /* OKENV_ACTOR_SAMPLE | _GREEDY | _EPS_GREEDY                      */
    float    epsilon;            /* [0, 1]; read by OKENV_ACTOR_EPS_GREEDY only                     */
    uint32_t seed, agent_base;   /* key of the draws; global id of the handle's agent 0             */
    float    action_table[8][2]; /* (throttle_delta, steering_delta) per action index (kActionMap)  */
} okenv_actor_params;

/* Where okenv_actor_act leaves this step's sample, besides the action fields: device pointers, each may be NULL (skipped). */
typedef struct okenv_actor_record {
    float   *state;  /* [N][R]  x, the networks' input (dist / kSensorRange)                                  */
    int64_t *action; /* [N]     the chosen index (what torch.gather wants)                                    */
    float   *prob;   /* [N]     the clamped probability of that action; in OKENV_ACTOR_EPS_GREEDY its logit   */
    float   *value;  /* [N]     the value network's output (left alone without a value network)               */
    uint8_t *alive;  /* [N]     !crashed_                                                                     */
} okenv_actor_record;

/* Attaches an actor to the handle (replaces an earlier one, whose parameters are forgotten).  The fan has at most 64 rays.
 * OKENV_ERR_INVALID for NULL arguments, a width or action count outside the limits above, an unknown mode, epsilon outside [0, 1]
 * (or NaN), more than 64 rays. */
OKENV_API int okenv_actor_create(okenv_t h, const okenv_actor_params *params);
/* Floats of the two parameter vectors, in the order of torch's parameters(): l1.weight [H][R] row-major, l1.bias [H], l2.weight
 * [A][H], l2.bias [A]; the value network's likewise with one output (0 floats without one).  Either pointer may be NULL. */
OKENV_API int okenv_actor_num_params(okenv_t h, int32_t *policy, int32_t *value);
/* New parameters from host or device pointers (a device pointer is a device-to-device copy on the handle's stream: the flattened
 * parameters of a torch module can be handed over after every optimiser step without a host hop).  A NULL pointer leaves that
 * network as it is.  No synchronisation: a host buffer must stay valid until the stream has passed the copy. */
OKENV_API int okenv_actor_set_params(okenv_t h, const float *policy, const float *value);
OKENV_API int okenv_actor_set_epsilon(okenv_t h, float epsilon);
/* A device word that is added to the draw index of every later okenv_actor_act (NULL: none).  For replayed HIP graphs of a handle
 * WITHOUT auto-reset, see okenv_actor_act. */
OKENV_API int okenv_actor_set_draw_offset(okenv_t h, const uint32_t *device_word);
/* updateAction for every agent, crashed ones included (ppo_sim.cpp:63-69 asks every agent): reads OKENV_F_DIST and crashed_, writes
 * OKENV_F_THROTTLE / OKENV_F_STEER and, when `rec` is given, the record slots.  One kernel on the handle's stream, no
 * synchronisation, no allocation: it can be captured into a HIP graph next to okenv_step (the contract of okenv_expert_act; like it,
 * it ends a running episode without the end-of-episode corrections).
 * The draw index is the handle's step count (okenv_get_step_count), which the call reads and does not advance: the agents draw
 * afresh after every step, and a population sharded over handles (agent_base) draws what the unsharded one draws.  While
 * auto-reset is on, the step count lives on the device (the step kernels advance it; it is the epoch of the reset draws) and the
 * kernel reads it there, so replays of a captured graph keep drawing fresh numbers.  Without auto-reset the step kernels leave the
 * device word alone and the host's count is passed by value: a captured launch then repeats its draw index on every replay, unless
 * the caller advances a word of its own inside the graph and registers it with okenv_actor_set_draw_offset.
 * OKENV_ERR_STATE before okenv_actor_create, or before okenv_actor_set_params has given every attached network its parameters. */
OKENV_API int okenv_actor_act(okenv_t h, const okenv_actor_record *rec);
/* The same rule on host arrays, no GPU needed: n agents (global ids params->agent_base + i), dist [n][num_rays], crashed [n] or
 * NULL.  Outputs, each may be NULL: throttle, steer, action, prob [n], value_out [n] (needs a value network), state [n][num_rays],
 * alive [n]. */
OKENV_API int okenv_actor_act_host(const okenv_actor_params *params, const float *policy, const float *value, int32_t num_rays, int32_t n,
                                   const float *dist, const uint8_t *crashed, uint32_t draw_index, float *throttle, float *steer,
                                   int64_t *action, float *prob, float *value_out, float *state, uint8_t *alive);

/* ---- from a recorded episode to the learner's batch ------------------------------------------------------
 * The data side of the reference's updatePolicy (RLRacers/PPO/ExperienceBuffer.hpp:15-68, ReinforceAgent.hpp:94-106,
 * GCLAgent.hpp:75-84,137-148) for a record of T step rows and N agent columns, as okenv_actor_act leaves it: discounted returns per
 * agent column with `alive` as the episode boundary, optionally GAE(lambda) advantages from the recorded values, their statistics
 * over the alive samples in an order no launch shape can change, the normalisation, and the alive samples packed densely in
 * step-major, agent-minor order.  The rule is written out in include/okenv_batch.h (ok_batch_*). */
#define OKENV_BATCH_NORMALIZE_RETURN 1u    /* the dense `ret` is (G - mean) / (std + FLT_EPSILON) */
#define OKENV_BATCH_NORMALIZE_ADVANTAGE 2u /* the dense `adv` likewise                            */

typedef struct okenv_batch_params {
    int32_t  num_steps;     /* T >= 1                                                                              */
    int32_t  num_agents;    /* N >= 1, T * N < 2^31 (not necessarily the handle's population)                     */
    int32_t  state_width;   /* R: floats per row of `state` (>= 1 when state is gathered)                          */
    int32_t  record_stride; /* agent slots between two rows of reward / alive / value; 0: N, else >= N             */
    int32_t  field_stride;  /* the same for state / action / prob                                                  */
    float    gamma;         /* [0, 1]                                                                              */
    float    lambda;        /* [0, 1]; read only with a value plane                                                */
    uint32_t normalize;     /* OKENV_BATCH_NORMALIZE_* bits                                                        */
    int32_t  block_threads; /* workgroup size of the column walk: 0 (the default, 64) or 64 / 128 / 256 / 512 / 1024;
                               no output depends on it                                                             */
} okenv_batch_params;

/* The record: device pointers (host pointers for okenv_batch_prepare_host).  reward and alive are required. */
typedef struct okenv_batch_input {
    const float   *reward;     /* [T][stride]      */
    const uint8_t *alive;      /* [T][stride]      non-zero: the agent produced this sample while driving */
    const float   *value;      /* [T][stride]      or NULL: no advantages */
    const float   *last_value; /* [N]              or NULL: the value after the last row, for columns still alive there */
    const float   *state;      /* [T][stride][R]   or NULL */
    const int64_t *action;     /* [T][stride]      or NULL */
    const float   *prob;       /* [T][stride]      or NULL: any per-sample fp32 field (the probability, or its logarithm) */
} okenv_batch_input;

/* Over the alive samples; sums in fp64, the order fixed by the rule.  The *_adv members are 0 without a value plane. */
typedef struct okenv_batch_stats {
    double  sum_ret, sumsq_ret, sum_adv, sumsq_adv;
    float   mean_ret, std_ret, mean_adv, std_adv; /* fp64 results rounded once; std is the unbiased estimate, 0 for M < 2 */
    int32_t count;                                /* M */
    int32_t reserved;
} okenv_batch_stats;

/* Where the batch goes: device pointers (host pointers for okenv_batch_prepare_host), each may be NULL (skipped).  The dense
 * outputs need room for T * N samples; their first M entries are written. */
typedef struct okenv_batch_output {
    float             *state;     /* [M][R]  needs input state                                               */
    int64_t           *action;    /* [M]     needs input action                                              */
    float             *prob;      /* [M]     needs input prob                                                */
    float             *ret;       /* [M]     G, normalised with OKENV_BATCH_NORMALIZE_RETURN                 */
    float             *adv;       /* [M]     A, normalised with OKENV_BATCH_NORMALIZE_ADVANTAGE; needs value */
    int32_t           *index;     /* [M]     t * N + i of sample k                                           */
    float             *ret_plane; /* [T][N]  G, never normalised, 0 where not alive                          */
    float             *adv_plane; /* [T][N]  A likewise; needs value                                         */
    okenv_batch_stats *stats;
    int32_t           *count;     /* M as a device word                                                      */
} okenv_batch_output;

/* Enqueues the whole preparation on the handle's stream: five kernels, no synchronisation, and no allocation after the first
 * call of a given T and N (the scratch belongs to the handle).  The handle lends its device, stream and scratch; the record is the
 * caller's.  OKENV_ERR_INVALID for a NULL handle, struct, reward or alive, T or N < 1, T * N >= 2^31, gamma or lambda NaN or
 * outside [0, 1], a stride smaller than N, unknown normalize bits, a block_threads not listed above, an output whose input is
 * missing (adv / adv_plane without value, state / action / prob without theirs, state with state_width < 1), last_value without
 * value. */
OKENV_API int okenv_batch_prepare(okenv_t h, const okenv_batch_params *params, const okenv_batch_input *in, const okenv_batch_output *out);
/* M of the handle's latest okenv_batch_prepare: waits for the stream and reads the one word the caller needs to size its views.
 * OKENV_ERR_STATE before the first okenv_batch_prepare. */
OKENV_API int okenv_batch_count(okenv_t h, int32_t *count);
/* The same rule on host arrays, no GPU needed; *count (may be NULL) receives M. */
OKENV_API int okenv_batch_prepare_host(const okenv_batch_params *params, const okenv_batch_input *in, const okenv_batch_output *out, int32_t *count);

/* ---- PPO's update: losses, gradients and Adam ------------------------------------------------------------
 * The minibatch loop of PPOAgent::updatePolicy (RLRacers/PPO/PPOAgent.hpp:109-151) on the batch okenv_batch_prepare leaves: per
 * minibatch the clipped-surrogate actor loss and the critic's squared error, their gradients through both networks, and one Adam
 * step on each, in place in the parameters okenv_actor_act reads.  The rule, with its summation order and torch autograd's
 * conventions, is written out in include/okenv_learn.h (ok_learn_*). */
typedef struct okenv_learner_params {
    float lr;    /* > 0 (kLearningRate 3e-4)  */
    float clip;  /* [0, 1) (kClip 0.2)        */
    float beta1; /* [0, 1), torch: 0.9        */
    float beta2; /* [0, 1), torch: 0.999      */
    float eps;   /* > 0, torch: 1e-8          */
} okenv_learner_params;

/* The training set: device pointers (host pointers for okenv_ppo_update_host). */
typedef struct okenv_ppo_batch {
    const float   *state;  /* [M][R]                                                                          */
    const int64_t *action; /* [M]                                                                             */
    const float   *prob;   /* [M]  the recorded clamped probability of the action (not its logarithm)         */
    const float   *ret;    /* [M]                                                                             */
    const float   *adv;    /* [M]  or NULL: ret - v(s), v from before the minibatch's steps (needs a critic)  */
} okenv_ppo_batch;

/* Where the update reports: device pointers (host pointers for okenv_ppo_update_host), each may be NULL (skipped). */
typedef struct okenv_ppo_output {
    float   *actor_loss;  /* [epochs * ceil(M / B)]  per minibatch                                            */
    float   *critic_loss; /* [epochs * ceil(M / B)]  0 without a critic                                       */
    int32_t *clipped;     /* [epochs * ceil(M / B)]  samples whose ratio left [1 - clip, 1 + clip]            */
    float   *grad_policy; /* the last minibatch's gradient of the actor loss, in parameter order              */
    float   *grad_value;  /* the last minibatch's gradient of the critic loss (left alone without a critic)   */
} okenv_ppo_output;

/* Parameters and Adam state on the host, read and written by okenv_ppo_update_host; the value_* members may be NULL without a
 * critic.  t: optimiser steps taken so far (one per minibatch, shared by both networks). */
typedef struct okenv_learner_state {
    float  *policy, *policy_m, *policy_v;
    float  *value, *value_m, *value_v;
    int64_t t;
} okenv_learner_state;

/* Attaches Adam state (m = v = 0, t = 0) for the networks of the handle's actor.  OKENV_ERR_STATE without an actor whose networks
 * all have their parameters; OKENV_ERR_INVALID for NULL arguments, lr <= 0, clip outside [0, 1), a beta outside [0, 1), eps <= 0
 * (or NaN). */
OKENV_API int okenv_learner_create(okenv_t h, const okenv_learner_params *params);
/* m = v = 0, t = 0 again.  (okenv_actor_set_params leaves the moments alone.) */
OKENV_API int okenv_learner_reset(okenv_t h);
/* Enqueues every minibatch of every epoch on the handle's stream, two kernels each (gradient partials per chunk; join + Adam on both
 * networks): no synchronisation, and no allocation after the first call of a given min(B, M).  `order` is a device array
 * [epochs][M] of int32 sample indices or NULL (sequential).  The next okenv_actor_act uses the new parameters.  The step number
 * advances per enqueued minibatch; if the call returns an error part of the way, call okenv_learner_reset or carry on from
 * okenv_learner_get_state's t, which counts the minibatches that were enqueued.
 * OKENV_ERR_STATE before okenv_learner_create; OKENV_ERR_INVALID for a NULL handle, batch, state, action, prob or ret, M, B or
 * epochs < 1, epochs * M >= 2^31, adv NULL without a critic. */
OKENV_API int okenv_ppo_update(okenv_t h, const okenv_ppo_batch *batch, int32_t M, int32_t B, int32_t epochs, const int32_t *order,
                               const okenv_ppo_output *out);
/* The same rule on host arrays, no GPU needed: networks num_rays -> hidden -> num_actions and num_rays -> value_hidden -> 1
 * (value_hidden 0: none). */
OKENV_API int okenv_ppo_update_host(const okenv_learner_params *params, int32_t num_rays, int32_t hidden, int32_t num_actions, int32_t value_hidden,
                                    okenv_learner_state *state, const okenv_ppo_batch *batch, int32_t M, int32_t B, int32_t epochs,
                                    const int32_t *order, const okenv_ppo_output *out);
/* The actor's parameters to host or device pointers (either may be NULL); synchronises.  OKENV_ERR_STATE before they were set. */
OKENV_API int okenv_actor_get_params(okenv_t h, float *policy, float *value);
/* The learner's moments to host or device pointers (each may be NULL) and its step number; synchronises. */
OKENV_API int okenv_learner_get_state(okenv_t h, float *policy_m, float *policy_v, float *value_m, float *value_v, int64_t *t);

/* ---- REINFORCE: the dropout actor and the whole-episode update --------------------------------------------
 * The reference's REINFORCE network as it is (RLRacers/Reinforce/Policy.hpp:22-29: Dropout between the first affine layer and the
 * ReLU, active while acting and in the update) and updatePolicy of ReinforceAgent.hpp:91-123 on the batch okenv_batch_prepare leaves:
 * loss = sum of -log p(a) * G over the episode's samples, its gradient through the masked network, one Adam step, in place in the
 * parameters okenv_actor_act reads.  The rule, with its Philox layout and summation order, is written out in
 * include/okenv_reinforce.h (ok_reinforce_*). */
#define OKENV_REINFORCE_SUM 0  /* loss and gradient are sums over the samples (the reference's loss +=) */
#define OKENV_REINFORCE_MEAN 1 /* each divided once by the number of samples of the step                */

/* Dropout with probability p on the hidden layer of the handle's POLICY network (never the value network), masks keyed by `seed`,
 * the global agent id and the draw index: okenv_actor_act then runs its dropout instantiation, and okenv_reinforce_update
 * regenerates every sample's mask.  The default is off (p = 0), and okenv_actor_create switches it off again.  While p > 0
 * okenv_ppo_update and okenv_dqn_update return OKENV_ERR_STATE: their forwards know no mask.  A captured okenv_actor_act carries p
 * and the seed by value.  OKENV_ERR_INVALID for a NULL handle, p outside [0, 1) or NaN, OKENV_ERR_STATE before
 * okenv_actor_create. */
OKENV_API int okenv_actor_set_dropout(okenv_t h, float p, uint32_t seed);
/* okenv_actor_act_host with dropout (p, dropout_seed); p == 0 is okenv_actor_act_host, bit for bit.  No GPU needed. */
OKENV_API int okenv_actor_act_dropout_host(const okenv_actor_params *params, float p, uint32_t dropout_seed, const float *policy, const float *value,
                                           int32_t num_rays, int32_t n, const float *dist, const uint8_t *crashed, uint32_t draw_index,
                                           float *throttle, float *steer, int64_t *action, float *prob, float *value_out, float *state,
                                           uint8_t *alive);

typedef struct okenv_reinforce_config {
    int32_t  accumulate; /* non-zero: ONE optimiser step per call, on the gradient of all M samples (the reference);
                            0: one step per slice of B samples (minibatch REINFORCE)                                   */
    int32_t  reduce;     /* OKENV_REINFORCE_SUM | _MEAN                                                                */
    int32_t  num_agents; /* N of the record the batch was cut from: sample index = row * N + agent (read with dropout) */
    uint32_t draw_first; /* the actor's draw index of the record's row 0 (read with dropout)                           */
} okenv_reinforce_config;

/* The training set: device pointers (host pointers for okenv_reinforce_update_host). */
typedef struct okenv_reinforce_batch {
    const float   *state;  /* [M][R]                                                                               */
    const int64_t *action; /* [M]                                                                                  */
    const float   *ret;    /* [M]  the (normalised) return G                                                       */
    const int32_t *index;  /* [M]  row * N + agent, as okenv_batch_prepare writes it; may be NULL while dropout is off */
} okenv_reinforce_batch;

/* Where the update reports: device pointers (host pointers for okenv_reinforce_update_host), each may be NULL (skipped). */
typedef struct okenv_reinforce_output {
    float *loss;        /* one value per optimiser step: 1 when accumulating, else ceil(M / B) */
    float *grad_policy; /* the last step's gradient, in parameter order                        */
} okenv_reinforce_output;

/* Enqueues the update on the handle's stream: the M samples in ceil(M / B) slices of B, two kernels per slice (gradient partials per
 * chunk; join + accumulate, or join + Adam), no synchronisation, and no allocation after the first call of a given min(B, M).  B only
 * bounds the scratch when accumulating: the sums' order, and so the result's bits, depend on it.  `order` is a device array [M] of
 * int32 sample indices or NULL (sequential).  The learner is the handle's (okenv_learner_create: lr, the betas and eps are read, clip
 * is not; t, m and v continue); the next okenv_actor_act uses the new parameters.
 * OKENV_ERR_STATE before okenv_learner_create; OKENV_ERR_INVALID for a NULL handle, config, batch, state, action or ret, M or B < 1, an
 * unknown reduce and, with dropout on, a NULL index or num_agents < 1. */
OKENV_API int okenv_reinforce_update(okenv_t h, const okenv_reinforce_config *config, const okenv_reinforce_batch *batch, int32_t M, int32_t B,
                                     const int32_t *order, const okenv_reinforce_output *out);
/* The same rule on host arrays, no GPU needed: network num_rays -> hidden -> num_actions, dropout (p, dropout_seed) with global agent
 * ids agent_base + index mod num_agents; of `state` the policy's members and t are read and written. */
OKENV_API int okenv_reinforce_update_host(const okenv_learner_params *params, const okenv_reinforce_config *config, float p, uint32_t dropout_seed,
                                          uint32_t agent_base, int32_t num_rays, int32_t hidden, int32_t num_actions, okenv_learner_state *state,
                                          const okenv_reinforce_batch *batch, int32_t M, int32_t B, const int32_t *order,
                                          const okenv_reinforce_output *out);

/* ---- Deep-Q learning: replay ring, sampling and the temporal-difference update ---------------------------
 * The learning side of RLRacers/Deep_Q_Learning (dq_racer_sim.cpp:81-132, DQAgent.hpp:106-181, common/ReplayBuffer.hpp) for the
 * handle's OKENV_ACTOR_EPS_GREEDY actor: a ring of transitions that persists across episodes on the device, filled by one push per
 * step, and updateDQN's iterations -- uniform samples, y = r + gamma max q'(s'), the mean squared error over B * A elements, its
 * gradient and one Adam step -- in place in the parameters okenv_actor_act reads.  The rule is written out in include/okenv_dqn.h
 * (ok_dqn_*).  The Q network is the actor's policy network R -> H -> A; a value network, if attached, is left alone. */
#define OKENV_REPLAY_PUSH_ALL 1u /* push every agent (the reference's loop), not only those that entered the step alive */
#define OKENV_DQN_MASK_DONE 1u   /* y = r + ((1 - done) * gamma) * max q' (DQAgent.hpp:134) instead of r + gamma * max q' (:133) */

/* The ring's fields: device pointers, or host pointers where a call says so; [C] slots each. */
typedef struct okenv_replay_ring {
    float   *state;      /* [C][R]  the networks' input before the step  */
    float   *next_state; /* [C][R]  dist / kSensorRange after the step   */
    int64_t *action;     /* [C]     the chosen index                     */
    float   *reward;     /* [C]                                          */
    float   *done;       /* [C]     1.0f: crashed_ after the step, else 0.0f */
} okenv_replay_ring;

typedef struct okenv_dqn_config {
    float    gamma;          /* [0, 1] (kGamma 0.99)                                                                        */
    uint32_t flags;          /* OKENV_DQN_MASK_DONE                                                                         */
    int32_t  target_network; /* 0: q' from the online parameters (the reference); 1: from the copy okenv_dqn_sync_target makes */
    uint32_t seed;           /* key of the sampling draws                                                                   */
} okenv_dqn_config;

/* Where the update reports: device pointers (host pointers for okenv_dqn_update_host), each may be NULL (skipped). */
typedef struct okenv_dqn_output {
    float   *loss;        /* [iterations]  mse_loss of every iteration                    */
    float   *grad_policy; /* the last iteration's gradient, in parameter order            */
    int32_t *index;       /* [B]           the slots the last iteration sampled           */
} okenv_dqn_output;

/* Attaches a ring of `capacity` slots to the handle (replaces an earlier one, whose contents are forgotten): every field zero,
 * pushed = 0.  All of the push's device memory is allocated here.  OKENV_ERR_INVALID for a NULL handle, capacity < 1, unknown flags,
 * more than 64 rays.  Synchronises.  The earlier ring's memory is freed: a HIP graph that captured
 * okenv_replay_push against it must not be replayed again. */
OKENV_API int okenv_replay_create(okenv_t h, int32_t capacity, uint32_t flags);
/* pushed = 0 again (the slots keep their bytes; nothing reads them).  OKENV_ERR_STATE before okenv_replay_create. */
OKENV_API int okenv_replay_reset(okenv_t h);
/* Appends the transitions of the step that has just run: `rec` is the record the preceding okenv_actor_act wrote (state and action are
 * required, alive unless OKENV_REPLAY_PUSH_ALL); next_state, done and the clearance reward come from the handle's fields after the
 * step; `reward` is NULL or a device array [N] that replaces the clearance reward.  Two short kernels on the handle's stream, no
 * synchronisation, no allocation: it can be captured into a HIP graph beside okenv_actor_act and okenv_step.
 * OKENV_ERR_STATE before okenv_replay_create; OKENV_ERR_INVALID for a NULL handle or record, or a record without state / action
 * (/ alive). */
OKENV_API int okenv_replay_push(okenv_t h, const okenv_actor_record *rec, const float *reward);
/* Transitions in the ring, min(pushed, capacity), and every transition ever pushed (either pointer may be NULL): waits for the stream
 * and reads the 8-byte word.  Nothing on the device path needs this. */
OKENV_API int okenv_replay_size(okenv_t h, int64_t *size, int64_t *pushed);
/* The ring's fields, all `capacity` slots of each, to host or device pointers (each may be NULL); synchronises. */
OKENV_API int okenv_replay_get(okenv_t h, const okenv_replay_ring *out);
/* The update's constants (before the first call: gamma 0.99, no flags, no target network, seed 0).  Turning the target network on
 * (from off: a call that leaves it on keeps the copy) allocates its copy and, when the actor has its parameters, fills it as
 * okenv_dqn_sync_target does; without parameters the update asks for okenv_dqn_sync_target.  A failed call changes nothing.  OKENV_ERR_INVALID for NULL
 * arguments, gamma NaN or outside [0, 1], unknown flags, target_network other than 0 or 1. */
OKENV_API int okenv_dqn_params(okenv_t h, const okenv_dqn_config *config);
/* `iterations` gradient steps on batches of B uniform samples of the ring, two kernels each on the handle's stream (gradient
 * partials per chunk of 32 positions, drawn and gathered straight from the ring; join + Adam): no synchronisation, and no allocation
 * after the first call of a given B.  Iteration i samples draw number draw_base + i with `resample`, else draw_base every time.  The
 * ring's size is read on the device.  The next okenv_actor_act uses the new parameters; the step number is the learner's.
 * OKENV_ERR_STATE before okenv_learner_create or okenv_replay_create, or with a target network that was never synchronised;
 * OKENV_ERR_INVALID for a NULL handle, B or iterations < 1, B * A >= 2^31. */
OKENV_API int okenv_dqn_update(okenv_t h, int32_t B, int32_t iterations, int32_t resample, uint32_t draw_base, const okenv_dqn_output *out);
/* Copies the online parameters into the target network, device to device on the handle's stream.  OKENV_ERR_STATE unless
 * okenv_dqn_params turned the target network on and the actor has its parameters. */
OKENV_API int okenv_dqn_sync_target(okenv_t h);
/* One push on host arrays, no GPU needed: ring of `capacity` slots (every field required) and *pushed, read and advanced; n agents with
 * the record's state [n][num_rays], action [n] and alive [n] (may be NULL with OKENV_REPLAY_PUSH_ALL), the distances [n][num_rays] and
 * crashed [n] after the step, reward [n] or NULL. */
OKENV_API int okenv_replay_push_host(const okenv_replay_ring *ring, int32_t capacity, int32_t num_rays, uint64_t *pushed, uint32_t flags, int32_t n,
                                     const float *state, const int64_t *action, const uint8_t *alive, const float *dist, const uint8_t *crashed,
                                     const float *reward);
/* The update on host arrays, no GPU needed: network num_rays -> hidden -> num_actions in state->policy / policy_m / policy_v / t (the
 * value members are not read), `target` the target network's parameters (required exactly when config->target_network is on), the
 * ring's fields and its size = min(pushed, capacity). */
OKENV_API int okenv_dqn_update_host(const okenv_learner_params *params, const okenv_dqn_config *config, int32_t num_rays, int32_t hidden,
                                    int32_t num_actions, okenv_learner_state *state, const float *target, const okenv_replay_ring *ring,
                                    int64_t size, int32_t B, int32_t iterations, int32_t resample, uint32_t draw_base,
                                    const okenv_dqn_output *out);

/* ---- DDPG: continuous actor, critic, replay ring and update -----------------------------------------------
 * RLRacers/DDPG (ddpg_sim.cpp:55-95, DDPGAgent.hpp:60-170) for every agent of the handle: an actor R -> H -> 2 that ends in
 * tanh * scale + bias and writes throttle_delta / steering_delta as real numbers, a critic (R + 2) -> Hc -> 1 on [state, action], two
 * target networks with soft updates, a ring whose action is two floats, and the update's iterations.  The rule is written out in
 * include/okenv_ddpg.h (ok_ddpg_*).  A DDPG object and a shared-network actor (okenv_actor_create) may live on one handle; neither
 * reads the other's buffers. */
typedef struct okenv_ddpg_config {
    int32_t  hidden;           /* H, 1 .. 256                                                       */
    int32_t  critic_hidden;    /* Hc, 1 .. 256                                                      */
    float    scale[2];         /* a_k = tanh(z_k) * scale_k + bias_k  (Actor.hpp: 50, 5)            */
    float    bias[2];          /*                                     (Actor.hpp: 50, 0)            */
    float    noise[2];         /* >= 0; 0: no exploration (the reference)                           */
    uint32_t seed, agent_base; /* key of the exploration draws; global id of the handle's agent 0   */
    float    gamma;            /* [0, 1] (kGamma 0.99)                                              */
    float    tau;              /* [0, 1] (kTau 0.005)                                               */
    float    lr_actor;         /* > 0 (1e-4)                                                        */
    float    lr_critic;        /* > 0 (1e-3)                                                        */
    float    beta1, beta2;     /* [0, 1), torch: 0.9, 0.999                                         */
    float    eps;              /* > 0, torch: 1e-8                                                  */
    uint32_t sample_seed;      /* key of the sampling draws                                         */
} okenv_ddpg_config;

/* Where okenv_ddpg_act leaves this step's sample, besides the action fields: device pointers, each may be NULL (skipped). */
typedef struct okenv_ddpg_record {
    float   *state;  /* [N][R]  x, the actor's input (dist / kSensorRange)  */
    float   *action; /* [N][2]  (throttle_delta, steering_delta)            */
    uint8_t *alive;  /* [N]     !crashed_                                   */
} okenv_ddpg_record;

/* The ring's fields: device pointers, or host pointers where a call says so; [C] slots each. */
typedef struct okenv_ddpg_ring {
    float *state;      /* [C][R] */
    float *next_state; /* [C][R] */
    float *action;     /* [C][2] */
    float *reward;     /* [C]    */
    float *done;       /* [C]    1.0f: crashed_ after the step, else 0.0f */
} okenv_ddpg_ring;

/* Parameters, target networks and Adam state: host or device pointers where a call says so.  t: iterations so far (both networks
 * step once per iteration). */
typedef struct okenv_ddpg_state {
    float  *actor, *critic, *actor_target, *critic_target;
    float  *actor_m, *actor_v, *critic_m, *critic_v;
    int64_t t;
} okenv_ddpg_state;

/* Where the update reports: device pointers (host pointers for okenv_ddpg_update_host), each may be NULL (skipped). */
typedef struct okenv_ddpg_output {
    float   *critic_loss; /* [iterations]  mse_loss of every iteration                  */
    float   *actor_loss;  /* [iterations]  -mean q of every iteration                   */
    float   *grad_critic; /* the last iteration's gradient, in parameter order          */
    float   *grad_actor;  /* the last iteration's gradient, in parameter order          */
    int32_t *index;       /* [B]           the slots the last iteration sampled         */
} okenv_ddpg_output;

/* Attaches a DDPG object to the handle (replaces an earlier one: parameters, moments and t are forgotten; a ring stays).  All device
 * memory of acting and of the networks is allocated here.  OKENV_ERR_INVALID for NULL arguments, a width outside 1 .. 256, more than
 * 62 rays, gamma or tau outside [0, 1] (or NaN), negative (or NaN) noise, lr or eps <= 0, a beta outside [0, 1). */
OKENV_API int okenv_ddpg_create(okenv_t h, const okenv_ddpg_config *config);
/* Floats of the two parameter vectors: actor [H][R], [H], [2][H], [2]; critic [Hc][R + 2], [Hc], [1][Hc], [1]. */
OKENV_API int okenv_ddpg_num_params(okenv_t h, int32_t *actor, int32_t *critic);
/* New online parameters from host or device pointers (NULL: left alone).  Each network that arrives also replaces its target network
 * (DDPGAgent.hpp:65-74).  Moments and t are left alone.  No synchronisation. */
OKENV_API int okenv_ddpg_set_params(okenv_t h, const float *actor, const float *critic);
/* Every non-NULL member of `out` is filled from the device (host or device pointers); out->t is set; synchronises.
 * OKENV_ERR_STATE before both networks have their parameters. */
OKENV_API int okenv_ddpg_get_state(okenv_t h, okenv_ddpg_state *out);
/* A device word added to the draw index of every later okenv_ddpg_act (NULL: none): okenv_actor_set_draw_offset's contract. */
OKENV_API int okenv_ddpg_set_draw_offset(okenv_t h, const uint32_t *device_word);
/* The action of every agent, crashed ones included: reads OKENV_F_DIST and crashed_, writes OKENV_F_THROTTLE / OKENV_F_STEER and the
 * record.  One kernel on the handle's stream, no synchronisation, no allocation: capturable beside okenv_step; ends a running
 * episode as okenv_actor_act does.  The draw index is okenv_actor_act's.  OKENV_ERR_STATE before the actor has its parameters. */
OKENV_API int okenv_ddpg_act(okenv_t h, const okenv_ddpg_record *rec);
/* The ring: okenv_replay_create / _reset / _push / _size / _get's contracts with a two-float action.  `reward` is NULL (1.0f per
 * transition, ddpg_sim.cpp:73) or a device array [N].  Needs 1 .. 62 rays. */
OKENV_API int okenv_ddpg_replay_create(okenv_t h, int32_t capacity, uint32_t flags);
OKENV_API int okenv_ddpg_replay_reset(okenv_t h);
OKENV_API int okenv_ddpg_replay_push(okenv_t h, const okenv_ddpg_record *rec, const float *reward);
OKENV_API int okenv_ddpg_replay_size(okenv_t h, int64_t *size, int64_t *pushed);
OKENV_API int okenv_ddpg_replay_get(okenv_t h, const okenv_ddpg_ring *out);
/* `iterations` iterations on batches of B uniform samples of the ring, four kernels each on the handle's stream (critic gradient
 * partials; join + Adam + soft update of the critic; actor gradient partials through the stepped critic; join + Adam + soft update
 * of the actor): no synchronisation, and no allocation after the first call of a given B.  The next okenv_ddpg_act uses the new
 * parameters.  OKENV_ERR_STATE before okenv_ddpg_create, before both networks have parameters, or before okenv_ddpg_replay_create;
 * OKENV_ERR_INVALID for a NULL handle, B or iterations < 1. */
OKENV_API int okenv_ddpg_update(okenv_t h, int32_t B, int32_t iterations, int32_t resample, uint32_t draw_base, const okenv_ddpg_output *out);
/* The same rules on host arrays, no GPU needed.  Act: n agents (global ids config->agent_base + i), dist [n][num_rays], crashed [n]
 * or NULL; outputs, each may be NULL: throttle, steer [n], action [n][2], state [n][num_rays], alive [n]. */
OKENV_API int okenv_ddpg_act_host(const okenv_ddpg_config *config, const float *actor, int32_t num_rays, int32_t n, const float *dist,
                                  const uint8_t *crashed, uint32_t draw_index, float *throttle, float *steer, float *action, float *state,
                                  uint8_t *alive);
OKENV_API int okenv_ddpg_replay_push_host(const okenv_ddpg_ring *ring, int32_t capacity, int32_t num_rays, uint64_t *pushed, uint32_t flags,
                                          int32_t n, const float *state, const float *action, const uint8_t *alive, const float *dist,
                                          const uint8_t *crashed, const float *reward);
/* Every member of `state` is required; size = min(pushed, capacity). */
OKENV_API int okenv_ddpg_update_host(const okenv_ddpg_config *config, int32_t num_rays, okenv_ddpg_state *state, const okenv_ddpg_ring *ring,
                                     int64_t size, int32_t B, int32_t iterations, int32_t resample, uint32_t draw_base,
                                     const okenv_ddpg_output *out);

/* ---- Continuous REINFORCE: two-hidden-layer Gaussian actor and whole-episode update ---------------------------
 * RLRacers/ReinforceContinuous (Policy.hpp:17-53, ReinforceAgent.hpp:49-146) for every agent of the handle: a network
 * R -> H1 -> H2 -> 2 with a free log_std [2], the action tanh(mu + exp(log_std) * eps) * scale + bias with eps a Box-Muller normal, its
 * log-probability, and updatePolicy on the batch okenv_batch_prepare leaves.  The rule is written out in include/okenv_gauss.h
 * (ok_gauss_*).  A Gaussian actor, a shared-network actor (okenv_actor_create) and a DDPG object may live on one handle; they share no
 * buffer.  The parameter vector is [log_std | fc1.weight | fc1.bias | fc2.weight | fc2.bias | mean.weight | mean.bias]: torch's
 * parameters() order for the reference's module. */
#define OKENV_GAUSS_GRAD_REFERENCE 0 /* the gradient autograd gives for the reference's graph (pre not detached) */
#define OKENV_GAUSS_GRAD_SCORE 1     /* the score-function estimator (pre detached)                              */

typedef struct okenv_gauss_config {
    int32_t  hidden1, hidden2; /* H1, H2: 1 .. 128; the gradient kernel's LDS (okenv_gauss_lds_bytes) must fit 160 KB */
    float    scale[2];         /* a_k = tanh(pre_k) * scale_k + bias_k  (the reference: 50, 10)                       */
    float    bias[2];          /*                                       (the reference: 50, 0)                        */
    int32_t  greedy;           /* 0: sample; 1: tanh(mu), no draw (ReinforceAgent.hpp:137-146)                        */
    uint32_t seed, agent_base; /* key of the normal draws; global id of the handle's agent 0                          */
} okenv_gauss_config;

/* Where okenv_gauss_act leaves this step's sample, besides the action fields: device pointers, each may be NULL (skipped). */
typedef struct okenv_gauss_record {
    float   *state;  /* [N][R]  x, the network's input (dist / kSensorRange)       */
    float   *eps;    /* [N][2]  the normal draws (not written when acting greedily) */
    float   *pre;    /* [N][2]  mu + std * eps (greedy: mu)                        */
    float   *action; /* [N][2]  (throttle_delta, steering_delta)                   */
    float   *logp;   /* [N]     the sample's log-probability                       */
    uint8_t *alive;  /* [N]     !crashed_                                          */
} okenv_gauss_record;

/* Parameters and Adam state: host or device pointers where a call says so; t: optimiser steps so far. */
typedef struct okenv_gauss_state {
    float  *params, *m, *v;
    int64_t t;
} okenv_gauss_state;

typedef struct okenv_gauss_update_config {
    int32_t accumulate; /* okenv_reinforce_config's: != 0 one Adam step per call on the slices' sum; 0 one step per slice */
    int32_t reduce;     /* OKENV_REINFORCE_SUM | _MEAN                                                               */
    int32_t grad_mode;  /* OKENV_GAUSS_GRAD_REFERENCE | _SCORE                                                        */
} okenv_gauss_update_config;

/* The batch: device pointers (host pointers for okenv_gauss_update_host).  eps is required in REFERENCE mode, pre in SCORE mode; the
 * other may be NULL. */
typedef struct okenv_gauss_batch {
    const float *state; /* [M][R] */
    const float *eps;   /* [M][2] */
    const float *pre;   /* [M][2] */
    const float *ret;   /* [M]    */
} okenv_gauss_batch;

/* Where the update reports: device pointers (host pointers for okenv_gauss_update_host), each may be NULL (skipped). */
typedef struct okenv_gauss_output {
    float *loss; /* [steps]  the loss of every optimiser step of the call */
    float *grad; /* the last step's gradient, in parameter order          */
} okenv_gauss_output;

/* LDS bytes of the gradient kernel for a network R -> H1 -> H2 -> A with chunks of 32 samples: a pure host function.  A shape is
 * accepted by okenv_gauss_create (and the host entries) only if this fits 160 KB; the chunk is never shrunk, because it is part of
 * the summation order.  0 for a width outside the rule's limits. */
OKENV_API int64_t okenv_gauss_lds_bytes(int32_t num_rays, int32_t hidden1, int32_t hidden2, int32_t num_actions);
/* Attaches a Gaussian actor to the handle (replaces an earlier one: parameters, moments and t are forgotten).  All device memory of
 * acting and of the network is allocated here.  OKENV_ERR_INVALID for NULL arguments, a width outside 1 .. 128, a shape whose gradient
 * kernel does not fit the LDS, greedy other than 0 or 1, a scale or bias that is not finite. */
OKENV_API int okenv_gauss_create(okenv_t h, const okenv_gauss_config *config);
OKENV_API int okenv_gauss_num_params(okenv_t h, int32_t *num_params);
/* New parameters from a host or device pointer; moments and t are left alone.  No synchronisation. */
OKENV_API int okenv_gauss_set_params(okenv_t h, const float *params);
/* The parameters to a host or device pointer; synchronises. */
OKENV_API int okenv_gauss_get_params(okenv_t h, float *params);
/* Every non-NULL member of `out` is filled from the device (host or device pointers); out->t is set; synchronises.  The moments exist
 * after okenv_gauss_learner_create (zeros before). */
OKENV_API int okenv_gauss_get_state(okenv_t h, okenv_gauss_state *out);
/* A device word added to the draw index of every later okenv_gauss_act (NULL: none): okenv_actor_set_draw_offset's contract. */
OKENV_API int okenv_gauss_set_draw_offset(okenv_t h, const uint32_t *device_word);
OKENV_API int okenv_gauss_set_greedy(okenv_t h, int32_t greedy);
/* The action of every agent, crashed ones included (okenv_ddpg_act's contract): reads OKENV_F_DIST and crashed_, writes
 * OKENV_F_THROTTLE / OKENV_F_STEER and the record.  One kernel on the handle's stream, no synchronisation, no allocation: capturable
 * beside okenv_step.  The draw index is okenv_actor_act's.  OKENV_ERR_STATE before the actor has its parameters. */
OKENV_API int okenv_gauss_act(okenv_t h, const okenv_gauss_record *rec);
/* The optimiser of the Gaussian actor: Adam's moments zeroed, t = 0.  `clip` is not read.  OKENV_ERR_STATE before the actor has its
 * parameters. */
OKENV_API int okenv_gauss_learner_create(okenv_t h, const okenv_learner_params *params);
/* okenv_reinforce_update's contract for this network: two kernels per slice on the handle's stream, no synchronisation, no allocation
 * after the first call of a given B; `order` [M] int32 on the device or NULL.  OKENV_ERR_STATE before okenv_gauss_learner_create;
 * OKENV_ERR_INVALID for NULL arguments, M or B < 1, an unknown reduce or grad_mode, a batch without state, ret or the mode's field. */
OKENV_API int okenv_gauss_update(okenv_t h, const okenv_gauss_update_config *config, const okenv_gauss_batch *batch, int32_t M, int32_t B,
                                 const int32_t *order, const okenv_gauss_output *out);
/* The same rules on host arrays, no GPU needed.  Act: n agents (global ids config->agent_base + i), dist [n][num_rays], crashed [n] or
 * NULL; outputs, each may be NULL: throttle, steer [n], eps, pre, action [n][2], logp [n], state [n][num_rays], alive [n]. */
OKENV_API int okenv_gauss_act_host(const okenv_gauss_config *config, const float *params, int32_t num_rays, int32_t n, const float *dist,
                                   const uint8_t *crashed, uint32_t draw_index, float *throttle, float *steer, float *eps, float *pre, float *action,
                                   float *logp, float *state, uint8_t *alive);
/* Network num_rays -> hidden1 -> hidden2 -> num_actions (1 .. 8 here: eps and pre are [M][num_actions]); every member of `state` is
 * required. */
OKENV_API int okenv_gauss_update_host(const okenv_learner_params *params, const okenv_gauss_update_config *config, int32_t num_rays, int32_t hidden1,
                                      int32_t hidden2, int32_t num_actions, okenv_gauss_state *state, const okenv_gauss_batch *batch, int32_t M,
                                      int32_t B, const int32_t *order, const okenv_gauss_output *out);

/* ---- Guided cost learning: cost, policy and value networks ---------------------------------------------------
 * RLRacers/GuidedCostLearning (Networks.hpp, GCLAgent.hpp, main.cpp:114-187, ReadExpertData.hpp) for every agent of the handle: a
 * Gaussian actor R -> H1 -> H2 -> 2 whose mean is squashed, a value network R -> H1 -> H2 -> 1 and a tanh cost network
 * (R + 2) -> C1 -> C2 -> 1 on [state | squashed action], with the state x_k = |sensor_hits_[k]|^2 / 200^2.  The rule is written out in
 * include/okenv_gcl.h (ok_gcl_*).  A GCL object, a shared-network actor, a Gaussian actor and a DDPG object may live on one handle;
 * they share no buffer.  Parameter vectors in torch's parameters() order: policy [log_std | fc1 | fc2 | fc3], value and cost
 * [fc1 | fc2 | fc3]. */
#define OKENV_GCL_POLICY 0
#define OKENV_GCL_VALUE 1
#define OKENV_GCL_COST 2

typedef struct okenv_gcl_config {
    int32_t  hidden1, hidden2;           /* H1, H2 of the policy and the value network: 1 .. 128                      */
    int32_t  cost_hidden1, cost_hidden2; /* C1, C2 of the cost network: 1 .. 128; its input R + 2 must not exceed 64  */
    float    scale[2];                   /* action_k = tanh(pre_k) * scale_k + bias_k  (the reference: 50, 10)        */
    float    bias[2];                    /*                                            (the reference: 50, 0)         */
    int32_t  greedy;                     /* 0: sample; 1: pre = mu, no draw                                           */
    uint32_t seed, agent_base;           /* key of the normal draws and of the expert draws; global id of agent 0     */
} okenv_gcl_config;

/* Where okenv_gcl_act leaves this step's sample, besides the action fields: device pointers, each may be NULL (skipped). */
typedef struct okenv_gcl_record {
    float   *state;    /* [N][R]  x_k = (rel_x^2 + rel_y^2) / 40000                    */
    float   *eps;      /* [N][2]  the normal draws (not written when acting greedily)  */
    float   *pre;      /* [N][2]  mu + std * eps (greedy: mu), before the squash       */
    float   *squashed; /* [N][2]  tanh(pre): the action the cost network reads         */
    float   *action;   /* [N][2]  (throttle_delta, steering_delta)                     */
    float   *logp;     /* [N]     the sample's log-probability, no tanh correction     */
    uint8_t *alive;    /* [N]     !crashed_                                            */
} okenv_gcl_record;

/* Parameters and Adam state of one network: host or device pointers where a call says so; t: optimiser steps so far. */
typedef struct okenv_gcl_state {
    float  *params, *m, *v;
    int64_t t;
} okenv_gcl_state;

/* The policy rows of a cost update: device pointers (host pointers for the host entry). */
typedef struct okenv_gcl_cost_batch {
    const float *state;    /* [Mp][R] */
    const float *squashed; /* [Mp][2] */
} okenv_gcl_cost_batch;

typedef struct okenv_gcl_cost_output {
    float *loss; /* [1]  BCEWithLogits(c_expert, 0) + BCEWithLogits(c_policy, 1) */
    float *grad; /* the step's gradient, in parameter order                      */
} okenv_gcl_cost_output;

typedef struct okenv_gcl_update_config {
    int32_t accumulate; /* okenv_reinforce_config's: != 0 one Adam step per call on the slices' sum; 0 one step per slice */
    int32_t reduce;     /* OKENV_REINFORCE_SUM | _MEAN                                                               */
} okenv_gcl_update_config;

/* The batch of a policy / value update: device pointers (host pointers for the host entry), all required. */
typedef struct okenv_gcl_batch {
    const float *state; /* [M][R] */
    const float *pre;   /* [M][2]  the recorded pre-squash sample */
    const float *logp;  /* [M]     the recorded log-probability   */
    const float *ret;   /* [M]     discounted returns G           */
} okenv_gcl_batch;

/* Where the update reports: device pointers (host pointers for the host entry), each may be NULL (skipped). */
typedef struct okenv_gcl_output {
    float   *policy_loss; /* [steps]  -mean (or -sum) of the clipped surrogate, per optimiser step */
    float   *value_loss;  /* [steps]  mean (or sum) of (v - G)^2                                   */
    int32_t *clipped;     /* [steps]  samples whose ratio left [1 - clip, 1 + clip]               */
    float   *grad_policy, *grad_value; /* the last step's gradients, in parameter order           */
    float   *adv;         /* [M]      the normalised advantages of the call                        */
} okenv_gcl_output;

/* LDS bytes of the largest of the three gradient kernels with chunks of 32 samples: a pure host function.  A shape is accepted only
 * if this fits 160 KB; the chunk is never shrunk, because it is part of the summation order.  0 for a width outside the rule's limits
 * (num_rays + 2 > 64 included). */
OKENV_API int64_t okenv_gcl_lds_bytes(int32_t num_rays, int32_t hidden1, int32_t hidden2, int32_t cost_hidden1, int32_t cost_hidden2);
/* Attaches a GCL object to the handle (replaces an earlier one: parameters, moments, step counts and the expert bank are forgotten).
 * OKENV_ERR_INVALID for NULL arguments, a width outside 1 .. 128, num_rays + 2 > 64, a shape that does not fit the LDS, greedy other
 * than 0 or 1, a scale or bias that is not finite. */
OKENV_API int okenv_gcl_create(okenv_t h, const okenv_gcl_config *config);
OKENV_API int okenv_gcl_num_params(okenv_t h, int32_t which, int32_t *num_params);
/* New parameters of network `which` (OKENV_GCL_POLICY | _VALUE | _COST) from a host or device pointer; moments and step counts are
 * left alone.  No synchronisation. */
OKENV_API int okenv_gcl_set_params(okenv_t h, int32_t which, const float *params);
/* The parameters to a host or device pointer; synchronises. */
OKENV_API int okenv_gcl_get_params(okenv_t h, int32_t which, float *params);
/* Every non-NULL member of `out` is filled from the device; out->t is the network's step count (policy and value share one);
 * synchronises. */
OKENV_API int okenv_gcl_get_state(okenv_t h, int32_t which, okenv_gcl_state *out);
/* A device word added to the draw index of every later okenv_gcl_act (NULL: none): okenv_actor_set_draw_offset's contract. */
OKENV_API int okenv_gcl_set_draw_offset(okenv_t h, const uint32_t *device_word);
OKENV_API int okenv_gcl_set_greedy(okenv_t h, int32_t greedy);
/* The action of every agent, crashed ones included: reads OKENV_F_REL_X / _REL_Y and crashed_, writes OKENV_F_THROTTLE /
 * OKENV_F_STEER and the record.  One kernel on the handle's stream, no synchronisation, no allocation: capturable beside okenv_step.
 * OKENV_ERR_STATE before the policy has its parameters. */
OKENV_API int okenv_gcl_act(okenv_t h, const okenv_gcl_record *rec);
/* The expert bank: E rows state [E][R] and action [E][2] (already in the network's units: ReadExpertData.hpp:98,111), copied from
 * device pointers on the handle's stream.  Allocates when E exceeds every earlier bank.  OKENV_ERR_INVALID for E < 1 or NULL. */
OKENV_API int okenv_gcl_set_expert(okenv_t h, const float *state, const float *action, int32_t E);
/* out[s] = cost([state_s | squashed_s]) for M rows, device pointers: one forward-only kernel, no synchronisation.  OKENV_ERR_STATE
 * before the cost network has its parameters. */
OKENV_API int okenv_gcl_cost(okenv_t h, const float *state, const float *squashed, int32_t M, float *out);
/* The optimisers: `policy_value` for the policy and the value network (its clip is the ratio's), `cost` for the cost network (its
 * clip is not read).  Moments zeroed, step counts 0.  OKENV_ERR_STATE before all three networks have their parameters. */
OKENV_API int okenv_gcl_learner_create(okenv_t h, const okenv_learner_params *policy_value, const okenv_learner_params *cost);
/* One Adam step of the cost network on Me expert positions drawn from the bank and the Mp policy rows of `batch`: a gradient kernel
 * and a join kernel on the handle's stream, no synchronisation, no allocation after the first call of a given size.
 * OKENV_ERR_STATE before okenv_gcl_learner_create or okenv_gcl_set_expert; OKENV_ERR_INVALID for NULL fields, Mp < 1 or Me < 1. */
OKENV_API int okenv_gcl_cost_update(okenv_t h, const okenv_gcl_cost_batch *batch, int32_t Mp, int32_t Me, const okenv_gcl_cost_output *out);
/* The advantages of the call (a forward-only sweep of the value network, their statistics, the normalisation), then the policy's
 * slices and the value's slices, two kernels each (okenv_reinforce_update's contract): no synchronisation, no allocation after the
 * first call of a given M and B; `order` [M] int32 on the device or NULL. */
OKENV_API int okenv_gcl_policy_update(okenv_t h, const okenv_gcl_update_config *config, const okenv_gcl_batch *batch, int32_t M, int32_t B,
                                      const int32_t *order, const okenv_gcl_output *out);
/* The same rules on host arrays, no GPU needed.  Act: n agents (global ids config->agent_base + i), rel_x, rel_y [n][num_rays],
 * crashed [n] or NULL; outputs, each may be NULL: throttle, steer [n], eps, pre, squashed, action [n][2], logp [n], state
 * [n][num_rays], alive [n]. */
OKENV_API int okenv_gcl_act_host(const okenv_gcl_config *config, const float *policy, int32_t num_rays, int32_t n, const float *rel_x,
                                 const float *rel_y, const uint8_t *crashed, uint32_t draw_index, float *throttle, float *steer, float *eps, float *pre,
                                 float *squashed, float *action, float *logp, float *state, uint8_t *alive);
OKENV_API int okenv_gcl_cost_host(const float *cost, int32_t num_rays, int32_t cost_hidden1, int32_t cost_hidden2, const float *state,
                                  const float *squashed, int32_t M, float *out);
/* Every member of `state` is required; state->t is the update number of the expert draws and advances by one. */
OKENV_API int okenv_gcl_cost_update_host(const okenv_learner_params *params, uint32_t seed, int32_t num_rays, int32_t cost_hidden1,
                                         int32_t cost_hidden2, okenv_gcl_state *state, const float *bank_state, const float *bank_action, int32_t E,
                                         const okenv_gcl_cost_batch *batch, int32_t Mp, int32_t Me, const okenv_gcl_cost_output *out);
/* Every member of both states is required; the step count is policy->t (value->t is set to it afterwards). */
OKENV_API int okenv_gcl_policy_update_host(const okenv_learner_params *params, const okenv_gcl_update_config *config, int32_t num_rays,
                                           int32_t hidden1, int32_t hidden2, okenv_gcl_state *policy, okenv_gcl_state *value,
                                           const okenv_gcl_batch *batch, int32_t M, int32_t B, const int32_t *order, const okenv_gcl_output *out);

/* ---- Lidar transformer driver -----------------------------------------------------------------------------
 * ImitationLearningTransformer (laser_transformer.py: LidarTransformer; infer_torch_traced_main.cpp) for every agent of the handle:
 * the hit points of the handle's rays, normalised, through a point embedding, post-norm transformer encoder layers and a control
 * head, to (throttle_delta, steering_delta).  Inference only.  The rule is written out in include/okenv_lidar.h (ok_lidar_*); the
 * linear layers run on the f32-input matrix cores.  The parameter vector is torch's parameters() order for the reference module
 * followed by a positional table pos [R][d_model] (ok_lidar_offsets). */
typedef struct okenv_lidar_config {
    int32_t num_points;      /* R: must equal the handle's ray count, 1 .. 16                                      */
    int32_t d_model;         /* multiple of 16, 16 .. 512        (the reference: 128)                              */
    int32_t nhead;           /* divides d_model                  (8)                                               */
    int32_t num_layers;      /* 1 .. 8                           (3)                                               */
    int32_t dim_feedforward; /* multiple of 16, 16 .. 4096       (512)                                             */
    int32_t head_hidden1;    /* multiple of 16, 16 .. 2048       (256)                                             */
    int32_t head_hidden2;    /* multiple of 16, 16 .. 2048       (64)                                              */
    float   action_lo[2];    /* a_k = (o_k + 1) / 2 * (hi_k - lo_k) + lo_k   (the reference: 0, -2)                */
    float   action_hi[2];    /*                                              (the reference: 100, 2)               */
    float   sensor_range;    /* points are normalised from [-sensor_range, sensor_range] to [-1, 1]  (200)          */
} okenv_lidar_config;

/* Where okenv_lidar_act leaves this step's sample, besides the action fields: device pointers, each may be NULL (skipped). */
typedef struct okenv_lidar_record {
    float   *action; /* [N][2]     (throttle_delta, steering_delta) */
    float   *input;  /* [N][R][2]  the normalised points            */
    uint8_t *alive;  /* [N]        !crashed_                        */
} okenv_lidar_record;

/* LDS bytes of the act kernel (16 agents per workgroup) for the shape: a pure host function.  A shape is accepted only if this fits
 * 160 KB.  0 for a NULL config or a shape outside the rule's limits. */
OKENV_API int64_t okenv_lidar_lds_bytes(const okenv_lidar_config *config);
/* Attaches a lidar policy to the handle (replaces an earlier one: its parameters are forgotten).  All device memory is allocated
 * here.  OKENV_ERR_INVALID for NULL arguments, num_points other than the handle's ray count, a width outside the limits above, a
 * shape that does not fit the LDS, ranges that are not finite or sensor_range <= 0. */
OKENV_API int okenv_lidar_create(okenv_t h, const okenv_lidar_config *config);
/* Floats of the parameter vector, the positional table included. */
OKENV_API int okenv_lidar_num_params(okenv_t h, int32_t *num_params);
/* New parameters from a host or device pointer.  No synchronisation. */
OKENV_API int okenv_lidar_set_params(okenv_t h, const float *params);
/* The parameters, in the same order, to a host or device pointer; synchronises. */
OKENV_API int okenv_lidar_get_params(okenv_t h, float *params);
/* The action of every agent, crashed ones included (okenv_expert_act's contract): reads OKENV_F_REL_X / _REL_Y and crashed_, writes
 * OKENV_F_THROTTLE / OKENV_F_STEER and the record.  One kernel on the handle's stream, no synchronisation, no allocation: capturable
 * beside okenv_step.  OKENV_ERR_STATE before okenv_lidar_create or okenv_lidar_set_params. */
OKENV_API int okenv_lidar_act(okenv_t h, const okenv_lidar_record *rec);
/* The same rule on host arrays, no GPU needed: n agents, rel_xy [n][R][2] (x, y interleaved), crashed [n] or NULL; outputs, each
 * may be NULL: throttle, steer [n], input [n][R][2], alive [n]. */
OKENV_API int okenv_lidar_act_host(const okenv_lidar_config *config, const float *params, int32_t n, const float *rel_xy, const uint8_t *crashed,
                                   float *throttle, float *steer, float *input, uint8_t *alive);
/* out [M][N] = x [M][K] w^T [N][K] + bias [N] (relu != 0: relu of it), the rule's linear layer alone.  On device `device` it runs
 * through the act kernel's own device function, 16 rows per workgroup; device < 0 (OKENV_DEBUG_ON_HOST) evaluates ok_lidar_dot on
 * the host.  Host pointers.  K and N multiples of 16, K <= 4096, N <= 4096; synchronises. */
OKENV_API int okenv_debug_lidar_linear(int32_t device, int32_t M, int32_t K, int32_t N, const float *x, const float *w, const float *bias,
                                       int32_t relu, float *out);

/* ---- Flow-matching driver ----------------------------------------------------------------------------------
 * FlowMatching (flow_matching_model.py: ActionFlowTrunk; main_flow_control.cpp:68-102) for every agent of the handle: from noise
 * x ~ N(0, I), `steps` Euler steps x += dt * trunk(x, t, cond) in one kernel, clamped to [-1, 1] and denormalised to
 * (throttle_delta, steering_delta).  cond is the image encoder's output for the agent; the encoder is the caller's.  Inference only.
 * The rule is written out in include/okenv_flow.h (ok_flow_*); the two wide linear layers run on the f32-input matrix cores.  The
 * parameter vector is torch's parameters() order for the reference's trunk (ok_flow_offsets). */
typedef struct okenv_flow_config {
    int32_t  cond_dim;         /* C: multiple of 16, 16 .. 512     (the reference: 128)                               */
    int32_t  hidden;           /* H: multiple of 16, 16 .. 512     (256)                                              */
    int32_t  steps;            /* S: Euler steps, 1 .. 256         (32)                                               */
    int32_t  noise;            /* 1: x starts from the normal draw; 0: from (0, 0), nothing is drawn                  */
    float    action_lo[2];     /* a_k = (x_k + 1) / 2 * (hi_k - lo_k) + lo_k, clamped to [lo_k, hi_k]  (0, -10)       */
    float    action_hi[2];     /*                                                                      (100, 10)      */
    uint32_t seed, agent_base; /* key of the normal draws; global id of the handle's agent 0                          */
} okenv_flow_config;

/* Where okenv_flow_act leaves this step's sample, besides the action fields: device pointers, each may be NULL (skipped). */
typedef struct okenv_flow_record {
    float   *x0;     /* [N][2]  the noise the sampler started from (zeros with noise == 0) */
    float   *x;      /* [N][2]  the clamped normalised sample                            */
    float   *action; /* [N][2]  (throttle_delta, steering_delta)                         */
    uint8_t *alive;  /* [N]     !crashed_                                                */
} okenv_flow_record;

/* LDS bytes of the act kernel for the shape: a pure host function.  A shape is accepted only if this fits 160 KB.  0 for a NULL
 * config or a shape outside the rule's limits. */
OKENV_API int64_t okenv_flow_lds_bytes(const okenv_flow_config *config);
/* Attaches a flow policy to the handle (replaces an earlier one: its parameters are forgotten).  All device memory is allocated
 * here.  OKENV_ERR_INVALID for NULL arguments, a width or step count outside the limits above, a shape that does not fit the LDS,
 * noise other than 0 or 1, ranges that are not finite. */
OKENV_API int okenv_flow_create(okenv_t h, const okenv_flow_config *config);
OKENV_API int okenv_flow_num_params(okenv_t h, int32_t *num_params);
/* New parameters from a host or device pointer.  No synchronisation. */
OKENV_API int okenv_flow_set_params(okenv_t h, const float *params);
/* The parameters, in the same order, to a host or device pointer; synchronises. */
OKENV_API int okenv_flow_get_params(okenv_t h, float *params);
/* A device word added to the draw index of every later okenv_flow_act (NULL: none): okenv_actor_set_draw_offset's contract. */
OKENV_API int okenv_flow_set_draw_offset(okenv_t h, const uint32_t *device_word);
/* The action of every agent, crashed ones included, from cond (device, [N][cond_dim]): reads crashed_, writes OKENV_F_THROTTLE /
 * OKENV_F_STEER and the record.  One kernel on the handle's stream, no synchronisation, no allocation: capturable beside okenv_step.
 * The draw index is okenv_actor_act's.  OKENV_ERR_STATE before okenv_flow_create or okenv_flow_set_params; OKENV_ERR_INVALID for a
 * NULL cond. */
OKENV_API int okenv_flow_act(okenv_t h, const float *cond, const okenv_flow_record *rec);
/* The same rule on host arrays, no GPU needed: n agents (global ids config->agent_base + i), cond [n][cond_dim], crashed [n] or NULL;
 * outputs, each may be NULL: throttle, steer [n], x0, x [n][2], alive [n]. */
OKENV_API int okenv_flow_act_host(const okenv_flow_config *config, const float *params, int32_t n, const float *cond, const uint8_t *crashed,
                                  uint32_t draw_index, float *throttle, float *steer, float *x0, float *x, uint8_t *alive);

/* ---- The flow driver's image encoder -----------------------------------------------------------------------
 * FlowMatching's BEVEncoder (flow_matching_model.py) for every agent of the handle: from the camera's RGBA8 frames
 * (okenv_render_views, rendered at image_size x image_size) the /255 normalisation, three stride-2 convolutions with ReLU, the global
 * average and the projection, to the [N][embed_dim] condition vectors okenv_flow_act takes.  Inference only.  The rule is written out
 * in include/okenv_bev.h (ok_bev_*); the convolutions run on the f32-input matrix cores.  The parameter vector is torch's
 * parameters() order for the reference's encoder (ok_bev_offsets); every weight must be finite. */
typedef struct okenv_bev_config {
    int32_t image_size;  /* S: multiple of 8, 16 .. 128                          (the reference: 128)         */
    int32_t kernel[3];   /* 3 or 5; stride 2 and padding kernel / 2              (5, 3, 3)                    */
    int32_t channels[3]; /* multiples of 16, 16 .. 128                           (32, 64, 128)                */
    int32_t embed_dim;   /* E: multiple of 16, 16 .. 512                         (128)                        */
} okenv_bev_config;

/* LDS bytes of the larger of the two conv kernels for the shape: a pure host function.  A shape is accepted only if this fits 160 KB.
 * 0 for a NULL config or a shape outside the rule's limits. */
OKENV_API int64_t okenv_bev_lds_bytes(const okenv_bev_config *config);
/* The sides (8 or 4) of the output tiles a workgroup of the first and of the second conv kernel owns for the shape: a pure host
 * function, what the tests name the kernels' paths by.  tiles [2]. */
OKENV_API int okenv_bev_tiles(const okenv_bev_config *config, int32_t *tiles);
/* Attaches an encoder to the handle (replaces an earlier one: its parameters are forgotten).  All device memory, the layers'
 * intermediate outputs included, is allocated here.  OKENV_ERR_INVALID for NULL arguments or a shape outside the limits above. */
OKENV_API int okenv_bev_create(okenv_t h, const okenv_bev_config *config);
OKENV_API int okenv_bev_num_params(okenv_t h, int32_t *num_params);
/* New parameters from a host or device pointer; the kernels' own copy of the conv weights is made behind it on the stream.  No
 * synchronisation. */
OKENV_API int okenv_bev_set_params(okenv_t h, const float *params);
/* The parameters, in the same order, to a host or device pointer; synchronises. */
OKENV_API int okenv_bev_get_params(okenv_t h, float *params);
/* out (device, [N][embed_dim]) from frames (device, 4-byte aligned, [N][S][S][4] uint8, frame_bytes = N S S 4 in all) for every
 * agent, crashed ones included.  Three kernels on the handle's stream, no synchronisation, no allocation: capturable beside
 * okenv_step, okenv_render_views and okenv_flow_act.  OKENV_ERR_STATE before okenv_bev_create or okenv_bev_set_params;
 * OKENV_ERR_INVALID for NULL pointers or another frame_bytes. */
OKENV_API int okenv_bev_encode(okenv_t h, const uint8_t *frames, int64_t frame_bytes, float *out);
/* okenv_bev_encode's kernels one by one, for measurement: only those named in `stages`, in their order (each reads what the one in
 * front of it left in the handle's buffers on an earlier call).  Refusals as okenv_bev_encode's. */
#define OKENV_BEV_STAGE_FRONT 1u /* layers 0 and 1 */
#define OKENV_BEV_STAGE_BACK 2u  /* layer 2 */
#define OKENV_BEV_STAGE_HEAD 4u  /* pool and projection */
OKENV_API int okenv_debug_bev_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, float *out, uint32_t stages);
/* The same rule on host arrays, no GPU needed: frames [n][S][S][4] -> out [n][embed_dim]. */
OKENV_API int okenv_bev_encode_host(const okenv_bev_config *config, const float *params, int32_t n, const uint8_t *frames, float *out);

/* ---- Behavioural-cloning image policy ----------------------------------------------------------------------
 * BehavioralCloning's PolicyCNN (env_train_bc.py) driven as main.cpp drives it, for every agent of the handle: from the camera's RGBA8
 * frames (okenv_render_views, rendered at image_size x image_size) the /255 normalisation, three valid convolutions with ReLU, the
 * flatten, a hidden layer with ReLU, one output and its tanh, to throttle_delta = throttle and steering_delta = steer_scale * output.
 * Inference only.  The rule is written out in include/okenv_cnn.h (ok_cnn_*); all matrix work runs on the f32-input matrix cores.  The
 * parameter vector is torch's parameters() order for the reference module (ok_cnn_offsets); every weight must be finite. */
typedef struct okenv_cnn_config {
    int32_t image_size;  /* S: 16 .. 128                                         (the reference: 96)          */
    int32_t kernel[3];   /* 1 .. 8; no padding                                   (8, 4, 3)                    */
    int32_t stride[3];   /* 1 .. 4, at most the kernel                           (4, 2, 1)                    */
    int32_t channels[3]; /* multiples of 16, 16 .. 128                           (32, 64, 64)                 */
    int32_t hidden;      /* H: multiple of 16, 16 .. 512                         (256)                        */
    float   throttle;    /* the constant throttle_delta; finite                  (100)                        */
    float   steer_scale; /* steering_delta per unit of the output; finite        (10)                         */
} okenv_cnn_config;

/* What an act can leave behind for the caller, device pointers, each may be NULL */
typedef struct okenv_cnn_record {
    float   *out;    /* [N]    the tanh output                         */
    float   *action; /* [N][2] throttle_delta, steering_delta          */
    uint8_t *alive;  /* [N]    1 where the agent was not crashed       */
} okenv_cnn_record;

/* LDS bytes of the larger of the two act kernels for the shape: a pure host function.  A shape is accepted only if this fits 160 KB.
 * 0 for a NULL config or a shape outside the rule's limits. */
OKENV_API int64_t okenv_cnn_lds_bytes(const okenv_cnn_config *config);
/* What names the kernels' path for the shape: a pure host function.  plan [2]: the tiles of 16 hidden units a wave of the head kernel
 * owns (1 .. 4: the head kernel's four forms), and what sizes the conv kernel's first LDS region (0: the frame, 1: layer 1's output). */
OKENV_API int okenv_cnn_plan(const okenv_cnn_config *config, int32_t *plan);
/* Attaches a policy to the handle (replaces an earlier one: its parameters are forgotten).  All device memory, the features between
 * the two kernels included, is allocated here.  OKENV_ERR_INVALID for NULL arguments, a shape outside the limits above or a
 * non-finite throttle or steer_scale. */
OKENV_API int okenv_cnn_create(okenv_t h, const okenv_cnn_config *config);
OKENV_API int okenv_cnn_num_params(okenv_t h, int32_t *num_params);
/* New parameters from a host or device pointer; the kernels' own copy of the weights is made behind it on the stream.  No
 * synchronisation. */
OKENV_API int okenv_cnn_set_params(okenv_t h, const float *params);
/* The parameters, in the same order, to a host or device pointer; synchronises. */
OKENV_API int okenv_cnn_get_params(okenv_t h, float *params);
/* Acts for every agent, crashed ones included, from frames (device, 4-byte aligned, [N][S][S][4] uint8, frame_bytes = N S S 4 in
 * all): writes OKENV_F_THROTTLE, OKENV_F_STEER and the record (rec may be NULL).  Two kernels on the handle's stream, no
 * synchronisation, no allocation: capturable beside okenv_step and okenv_render_views.  OKENV_ERR_STATE before okenv_cnn_create or
 * okenv_cnn_set_params; OKENV_ERR_INVALID for NULL frames or another frame_bytes. */
OKENV_API int okenv_cnn_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_cnn_record *rec);
/* okenv_cnn_act's kernels one by one, for measurement: only those named in `stages`, in their order (the head reads what the conv
 * kernel left in the handle's buffer on an earlier call).  Refusals as okenv_cnn_act's. */
#define OKENV_CNN_STAGE_CONV 1u /* layers 0, 1 and 2 */
#define OKENV_CNN_STAGE_HEAD 2u /* hidden layer, output and action */
OKENV_API int okenv_debug_cnn_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_cnn_record *rec, uint32_t stages);
/* The same rule on host arrays, no GPU needed: frames [n][S][S][4]; crashed [n] or NULL; every output [n] and may be NULL. */
OKENV_API int okenv_cnn_act_host(const okenv_cnn_config *config, const float *params, int32_t n, const uint8_t *frames, const uint8_t *crashed,
                                 float *throttle, float *steer, float *out, uint8_t *alive);

/* ---- World-model racers -------------------------------------------------------------------------------------
 * WorldModelVaeRnn/main.cpp's CmaEsAgent for every agent of the handle, each agent one CMA-ES candidate: from the camera's RGBA8
 * frames (okenv_render_views, rendered at image_size x image_size) the /255 normalisation, the conv-VAE encoder's four stride-2
 * convolutions (kernel 4, padding 1, eval-mode BatchNorm folded in) with ReLU and fc_mu, the state [mu | sin(rot), cos(rot)], the
 * agent's OWN controller (Z + 2 -> hidden -> hidden / 2 -> 1, tanh after each layer), to throttle_delta = throttle and
 * steering_delta = steer_scale * output; and the fitness of main.cpp:329-342.  Inference only.  The rule is written out in
 * include/okenv_world.h (ok_world_*); all matrix work runs on the f32-input matrix cores.  Two parameter vectors: the encoder's, shared
 * (ok_world_offsets), and the controllers', [N][ok_controller_num_params(latent + 2, hidden, 1)]; every weight must be finite. */
typedef struct okenv_world_config {
    int32_t image_size;   /* S: multiple of 16, 16 .. 128                        (the reference: 128)         */
    int32_t channels[4];  /* multiples of 16, 16 .. 512                          (64, 128, 256, 512)          */
    int32_t latent;       /* Z: multiple of 16, 16 .. 128; channels[3] (S/16)^2 <= 32768      (32)            */
    int32_t hidden;       /* the controller's: even, 2 .. 64                     (16)                         */
    float   throttle;     /* the constant throttle_delta; finite                 (100)                        */
    float   steer_scale;  /* steering_delta per unit of the output; finite       (5)                          */
    int32_t skip_crashed; /* 1: an act writes nothing for agents crashed at its time and spends no work on their frames */
} okenv_world_config;

/* What an act can leave behind for the caller, device pointers, each may be NULL */
typedef struct okenv_world_record {
    float   *mu;     /* [N][Z]     the encoder's mu                        */
    float   *state;  /* [N][Z + 2] mu, sin(rot), cos(rot)                  */
    float   *out;    /* [N]        the controller's output                 */
    float   *action; /* [N][2]     throttle_delta, steering_delta          */
    uint8_t *alive;  /* [N]        1 where the agent was not crashed       */
} okenv_world_record;

/* LDS bytes of the largest act kernel for the shape: a pure host function.  A shape is accepted only if this fits 160 KB.  0 for a
 * NULL config or a shape outside the rule's limits. */
OKENV_API int64_t okenv_world_lds_bytes(const okenv_world_config *config);
/* What names the kernels' path for the shape: a pure host function.  plan [12], three per convolution: the workgroups its output
 * channels take (128 a workgroup; waves of the last one idle where the count is no multiple of 128), the K blocks per tap (chunks of
 * up to 64 input channels; 0 for layer 0, whose whole chain is one block) and the channels of a tap's last block (16 .. 64). */
OKENV_API int okenv_world_plan(const okenv_world_config *config, int32_t *plan);
/* Device bytes okenv_world_create allocates for N agents (packed weights, controllers, the activations between the kernels, fitness). */
OKENV_API int64_t okenv_world_workspace_bytes(const okenv_world_config *config, int32_t num_agents);
/* Attaches the racers to the handle (replaces earlier ones: their parameters are forgotten; the fitness is zeroed).  All device memory
 * is allocated here.  OKENV_ERR_INVALID for NULL arguments, a shape outside the limits, a non-finite throttle or steer_scale or a
 * skip_crashed other than 0 or 1. */
OKENV_API int okenv_world_create(okenv_t h, const okenv_world_config *config);
/* Floats of the encoder vector and of ONE agent's controller. */
OKENV_API int okenv_world_num_params(okenv_t h, int32_t *encoder, int32_t *controller);
/* New parameters from a host or device pointer: `which` OKENV_WORLD_ENCODER (the kernels' own copy of the weights is made behind it on
 * the stream) or OKENV_WORLD_CONTROLLERS ([N][controller], one copy on the stream: cheap, it is called every generation).  No
 * synchronisation. */
#define OKENV_WORLD_ENCODER 0
#define OKENV_WORLD_CONTROLLERS 1
OKENV_API int okenv_world_set_params(okenv_t h, int32_t which, const float *params);
/* The parameters, in the same order, to a host or device pointer; synchronises. */
OKENV_API int okenv_world_get_params(okenv_t h, int32_t which, float *params);
/* Acts from frames (device, 4-byte aligned, [N][S][S][4] uint8, frame_bytes = N S S 4 in all): writes OKENV_F_THROTTLE, OKENV_F_STEER
 * and the record (rec may be NULL), for every agent, or with skip_crashed for those not crashed.  Kernels on the handle's stream only,
 * no synchronisation, no allocation: capturable beside okenv_step and okenv_render_views.  OKENV_ERR_STATE before okenv_world_create or
 * before both okenv_world_set_params; OKENV_ERR_INVALID for NULL frames or another frame_bytes. */
OKENV_API int okenv_world_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_world_record *rec);
/* The lane widths RaceTrack::getDistanceToLaneCenter divides by, host or device [P]; P must equal the centre line's. */
OKENV_API int okenv_world_set_lane_widths(okenv_t h, const float *w_left, const float *w_right, int32_t num_points);
/* The fitness: _begin zeroes it; _score is one kernel on the stream (capturable): per agent, not crashed: += 1 - distance to the lane
 * centre over the lane width; crashed and timed out: = 0.  OKENV_ERR_STATE before okenv_world_create (score: or set_lane_widths). */
OKENV_API int okenv_world_score_begin(okenv_t h);
OKENV_API int okenv_world_score(okenv_t h);
/* The fitness [N] to a host or device pointer (synchronises), and where it lives on the device. */
OKENV_API int okenv_world_fitness(okenv_t h, float *out);
OKENV_API int okenv_world_fitness_device(okenv_t h, float **ptr);
/* okenv_world_act's kernels one by one, for measurement: only those named in `stages`, in their order (each reads what the one before
 * left in the handle's buffers on an earlier call).  Refusals as okenv_world_act's. */
#define OKENV_WORLD_STAGE_LIST 1u
#define OKENV_WORLD_STAGE_CONV0 2u /* CONV0 << l: layer l */
#define OKENV_WORLD_STAGE_LATENT 32u
#define OKENV_WORLD_STAGE_HEAD 64u
OKENV_API int okenv_debug_world_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_world_record *rec, uint32_t stages);
/* The same rules on host arrays, no GPU needed.  act: frames [n][S][S][4], rot [n] (degrees, as stored), crashed [n] or NULL; the
 * outputs mu [n][Z], state [n][Z + 2], out, throttle, steer, alive [n], each may be NULL; with skip_crashed the entries of crashed
 * agents are left as they are.  score: one okenv_world_score on fitness [n] in place. */
OKENV_API int okenv_world_act_host(const okenv_world_config *config, const float *encoder, const float *controllers, int32_t n,
                                   const uint8_t *frames, const float *rot, const uint8_t *crashed, float *mu, float *state, float *out,
                                   float *throttle, float *steer, uint8_t *alive);
OKENV_API int okenv_world_score_host(const float *cx, const float *cy, const float *w_left, const float *w_right, int32_t num_points, int32_t n,
                                     const float *x, const float *y, const uint8_t *crashed, const uint8_t *timed_out, float *fitness);

/* ---- World-model racers' memory -----------------------------------------------------------------------------
 * The "M" of WorldModelVaeRnn's Vision + Memory + Controller: train_rnn.py's GRUDynamics (a stacked GRU on [z | a] with a linear head
 * that predicts the next latent) and main.cpp's CmaEsAgent::runVaeRnn, whose controllers read [z_t | h_top].  It attaches to a handle
 * that has okenv_world_create's racers and reuses their encoder, list and score; okenv_world_act itself is unchanged.  Every agent
 * carries a hidden state [layers][hidden] in the handle, from act to act.  The rule is written out in include/okenv_memory.h
 * (ok_memory_*), with its deliberate departures: the sums run in blocks of 64, the latent is mu, and `carry` chooses between the reference as
 * written (0: every act starts from a zero state) and the memory its Readme describes (1).  Two parameter vectors: the network's, shared
 * (ok_memory_offsets: torch's state_dict order of GRUDynamics, then z_mean, z_std, a_mean, a_std), and the controllers',
 * [N][ok_controller_num_params(latent + hidden, ctrl_hidden, 1)].  Every value must be finite and every std > 0. */
typedef struct okenv_memory_config {
    int32_t hidden;      /* H: multiple of 16, 16 .. 512                        (the reference: 512)         */
    int32_t layers;      /* L: 1 .. 4                                           (3)                          */
    int32_t ctrl_hidden; /* the controller's: even, 2 .. 64                     (16)                         */
    int32_t carry;       /* 1: the hidden state persists from act to act; 0: every act starts from zero      */
    float   throttle;    /* the constant throttle_delta; finite                 (100)                        */
    float   steer_scale; /* steering_delta per unit of the output; finite       (5)                          */
} okenv_memory_config;

/* What an act can leave behind for the caller, device pointers (okenv_memory_act_host: host pointers), each may be NULL */
typedef struct okenv_memory_record {
    float   *mu;         /* [N][Z]     the encoder's mu                                 */
    float   *hidden;     /* [N][H]     the top layer's hidden state after the act       */
    float   *prediction; /* [N][Z]     the head's next latent, denormalised             */
    float   *state;      /* [N][Z + H] mu, h_top: the controller's input                */
    float   *out;        /* [N]        the controller's output                          */
    float   *action;     /* [N][2]     throttle_delta, steering_delta                   */
    uint8_t *alive;      /* [N]        1 where the agent was not crashed                */
} okenv_memory_record;

/* LDS bytes of the largest memory kernel for the shape (`world` supplies the latent width): a pure host function.  0 for a NULL config
 * or a shape outside the limits.  Always inside 160 KB. */
OKENV_API int64_t okenv_memory_lds_bytes(const okenv_world_config *world, const okenv_memory_config *config);
/* What names the kernels' paths for the shape: a pure host function.  plan [8]: the column blocks of a layer (32 hidden units a
 * workgroup), the live column tiles of the last block (1 or 2), the K blocks of layer 0's input chain (64 k's a block) and the k's of the
 * last one, the K blocks of a chain over the hidden width and the k's of the last one, whether the Whh pass runs (carry), and the layer
 * kernel's launches. */
OKENV_API int okenv_memory_plan(const okenv_world_config *world, const okenv_memory_config *config, int32_t *plan);
/* Device bytes okenv_memory_create allocates for N agents (the network vector, its packed matrices, controllers, inputs, both hidden
 * buffers). */
OKENV_API int64_t okenv_memory_workspace_bytes(const okenv_world_config *world, const okenv_memory_config *config, int32_t num_agents);
/* Attaches the memory to the handle's racers (replaces an earlier one: its parameters are forgotten) and zeroes every hidden state.  All
 * device memory is allocated here.  OKENV_ERR_STATE before okenv_world_create; a later okenv_world_create detaches the memory.
 * OKENV_ERR_INVALID for NULL arguments, a shape outside the limits, a carry other than 0 or 1 or a non-finite throttle or steer_scale. */
OKENV_API int okenv_memory_create(okenv_t h, const okenv_memory_config *config);
/* Floats of the network vector and of ONE agent's controller. */
OKENV_API int okenv_memory_num_params(okenv_t h, int32_t *network, int32_t *controller);
/* New parameters from a host or device pointer: `which` OKENV_MEMORY_NETWORK (the kernels' own copy of the matrices is made behind it
 * on the stream) or OKENV_MEMORY_CONTROLLERS ([N][controller], one copy on the stream).  No synchronisation, so the values are not
 * looked at: okenv_memory_act_host is where a non-finite value or a std <= 0 is refused. */
#define OKENV_MEMORY_NETWORK 0
#define OKENV_MEMORY_CONTROLLERS 1
OKENV_API int okenv_memory_set_params(okenv_t h, int32_t which, const float *params);
/* The parameters, in the same order, to a host or device pointer; synchronises. */
OKENV_API int okenv_memory_get_params(okenv_t h, int32_t which, float *params);
/* Zeroes every agent's hidden state: one kernel on the handle's stream, capturable. */
OKENV_API int okenv_memory_reset(okenv_t h);
/* Every agent's hidden state [N][layers][hidden] from / to a host or device pointer, for tests and checkpoints.  set: a copy on the
 * stream, no synchronisation; get synchronises. */
OKENV_API int okenv_memory_set_hidden(okenv_t h, const float *hidden);
OKENV_API int okenv_memory_get_hidden(okenv_t h, float *hidden);
/* Acts from frames as okenv_world_act does (same frames, same refusals): reads OKENV_F_THROTTLE / OKENV_F_STEER as the action of the
 * step before, advances the hidden states, writes OKENV_F_THROTTLE, OKENV_F_STEER and the record (rec may be NULL), for every agent, or
 * with the racers' skip_crashed for those not crashed (a crashed agent keeps its hidden state).  Kernels on the handle's stream only, no
 * synchronisation, no allocation: capturable beside okenv_step, okenv_render_views and okenv_world_score.  OKENV_ERR_STATE before
 * okenv_memory_create, before the racers' encoder is set or before both okenv_memory_set_params. */
OKENV_API int okenv_memory_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_memory_record *rec);
/* okenv_memory_act's kernels one by one, for measurement: only those named in `stages`, in their order (each reads what the one before
 * left in the handle's buffers on an earlier call).  Refusals as okenv_memory_act's. */
#define OKENV_MEMORY_STAGE_ENCODER 1u /* okenv_world_act's list, convolutions and latent kernels */
#define OKENV_MEMORY_STAGE_INPUT 2u
#define OKENV_MEMORY_STAGE_LAYER0 4u /* LAYER0 << l: layer l */
#define OKENV_MEMORY_STAGE_HEAD 64u
OKENV_API int okenv_debug_memory_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_memory_record *rec, uint32_t stages);
/* The same rule on host arrays, no GPU needed: frames [n][S][S][4]; crashed [n] or NULL; hidden [n][layers][hidden], throttle and
 * steer [n] in and out (the stored action in, the new one out); rec: HOST pointers or NULL.  world: the racers' config (its shape and
 * skip_crashed; its hidden, throttle and steer_scale are not read).  With skip_crashed everything of a crashed agent is left as it is.
 * Refuses a network vector with a non-finite value or a std <= 0. */
OKENV_API int okenv_memory_act_host(const okenv_world_config *world, const okenv_memory_config *config, const float *encoder, const float *network,
                                    const float *controllers, int32_t n, const uint8_t *frames, const uint8_t *crashed, float *hidden,
                                    float *throttle, float *steer, const okenv_memory_record *rec);

/* ---- The memory's training ------------------------------------------------------------------------------------
 * train_rnn.py's recipe for the network of okenv_memory_create on the device: windows of seq_len steps over recorded latents and
 * actions, teacher forcing, mean squared error on the normalised next latent, backpropagation through time, clipping by the global
 * norm, AdamW.  The rule is written out in include/okenv_memtrain.h (ok_memtrain_*); every contraction runs on the f32-input matrix
 * cores.  The statistics at the network vector's end are not trained. */
typedef struct okenv_memory_learner_config {
    float   lr;           /* > 0; the rate of a minibatch without a schedule     (the reference: 1e-3) */
    float   beta1;        /* [0, 1), torch: 0.9                                                         */
    float   beta2;        /* [0, 1), torch: 0.999                                                       */
    float   eps;          /* > 0, torch: 1e-8                                                           */
    float   weight_decay; /* >= 0, AdamW's                                       (1e-4)                 */
    float   clip_grad;    /* >= 0, the global norm's limit; 0: no clipping       (1.0)                  */
    int32_t seq_len;      /* S: steps of a window, 1 .. 16                       (5)                    */
    int32_t max_batch;    /* the most windows a minibatch may hold               (256)                  */
} okenv_memory_learner_config;

/* The network vector (all of it, statistics included) and Adam's moments of its trainable prefix (the vector without its last
 * 2 Z + 4 floats); t: steps taken so far. */
typedef struct okenv_memory_learner_state {
    float  *params, *m, *v;
    int64_t t;
} okenv_memory_learner_state;

/* Where an update reports: device pointers (host pointers for okenv_memory_update_host), each may be NULL (skipped). */
typedef struct okenv_memory_learner_output {
    float *loss; /* [epochs * ceil(M / B)]  per minibatch, from before its step                        */
    float *norm; /* [epochs * ceil(M / B)]  the gradient's global norm before clipping                 */
    float *grad; /* the last minibatch's gradient after clipping, [trainable prefix]                   */
} okenv_memory_learner_output;

/* Device bytes okenv_memory_learner_create allocates, and the LDS bytes of its largest kernel (0: the kernels keep their operands in
 * registers): pure host functions.  0 for a NULL or refused argument. */
OKENV_API int64_t okenv_memory_learner_workspace_bytes(const okenv_world_config *world, const okenv_memory_config *config,
                                                       const okenv_memory_learner_config *learner);
OKENV_API int64_t okenv_memory_learner_lds_bytes(const okenv_world_config *world, const okenv_memory_config *config);
/* Attaches the learner (m = v = 0, t = 0) to the handle's memory; all its device memory is allocated here.  A later
 * okenv_memory_create or okenv_world_create drops it.  OKENV_ERR_STATE before okenv_memory_create or before the network's parameters
 * are set; OKENV_ERR_INVALID for NULL arguments or values outside the ranges above. */
OKENV_API int okenv_memory_learner_create(okenv_t h, const okenv_memory_learner_config *config);
/* m = v = 0, t = 0 again. */
OKENV_API int okenv_memory_learner_reset(okenv_t h);
/* The network vector and Adam's moments to host or device pointers (each may be NULL), and t; synchronises. */
OKENV_API int okenv_memory_learner_get_state(okenv_t h, okenv_memory_learner_state *out);
/* Enqueues every minibatch of every epoch on the handle's stream: no synchronisation, no allocation, capturable (the step number lives
 * on the device, so a replay takes the steps that follow).  latent [rows][Z], action [rows][2], start [M] (int32 rows): device; `order`
 * a device array [epochs][M] of int32 window indices or NULL (sequential); lr_schedule a HOST array [epochs * ceil(M / B)] or NULL (the
 * config's lr).  Step s of window w reads row start[w] + s * stride, and its target is the row a stride further; rows and indices
 * outside their range count as the nearest valid one.  Steps the handle's network vector in place and renews the act's copy of its
 * matrices: the next okenv_memory_act on the stream acts with the new network, okenv_memory_get_params returns it.  No agent field and
 * no hidden state is touched.  OKENV_ERR_STATE before okenv_memory_learner_create; OKENV_ERR_INVALID for a NULL handle or array, rows,
 * M, B or epochs < 1, B above max_batch (where M is above it too), epochs * M >= 2^31. */
OKENV_API int okenv_memory_update(okenv_t h, const float *latent, const float *action, int32_t rows, const int32_t *start, int32_t M, int32_t stride,
                                  int32_t B, int32_t epochs, const int32_t *order, const float *lr_schedule, const okenv_memory_learner_output *out);
/* The loss of every minibatch of one sequential pass with no step, to loss [ceil(M / B)] (device): the validation loop. */
OKENV_API int okenv_memory_eval(okenv_t h, const float *latent, const float *action, int32_t rows, const int32_t *start, int32_t M, int32_t stride, int32_t B,
                                float *loss);
/* The same rule on host arrays, no GPU needed.  Refuse a network vector with a non-finite value or a std <= 0. */
OKENV_API int okenv_memory_update_host(const okenv_world_config *world, const okenv_memory_config *config, const okenv_memory_learner_config *learner,
                                       okenv_memory_learner_state *state, const float *latent, const float *action, int32_t rows, const int32_t *start,
                                       int32_t M, int32_t stride, int32_t B, int32_t epochs, const int32_t *order, const float *lr_schedule,
                                       const okenv_memory_learner_output *out);
OKENV_API int okenv_memory_eval_host(const okenv_world_config *world, const okenv_memory_config *config, const okenv_memory_learner_config *learner,
                                     const float *network, const float *latent, const float *action, int32_t rows, const int32_t *start, int32_t M,
                                     int32_t stride, int32_t B, float *loss);
/* The update's forward of ONE window on the host, for tests: hidden [seq_len][layers][hidden] and zn [seq_len][Z], the hidden states
 * behind every step and the head's normalised predictions. */
OKENV_API int okenv_memory_window_host(const okenv_world_config *world, const okenv_memory_config *config, const float *network, const float *latent,
                                       const float *action, int32_t rows, int32_t start, int32_t stride, int32_t seq_len, float *hidden, float *zn);

/* ---- Deep-Q image racers ------------------------------------------------------------------------------------
 * RLRacers/DQN_CNN (CNN.hpp, DQCNNAgent.hpp, dq_cnn_racer_sim.cpp) for every agent of the handle: from the camera's RGBA8 frames
 * (okenv_render_views, rendered at image_size x image_size) one grey plane, three PADDED convolutions with ReLU, the flatten, fc1 with
 * ReLU, fc2 to num_actions Q-values, the greedy or epsilon-greedy choice of the shared-network actors and their action table; and the
 * ring of frame transitions with its push and its batch gather.  The temporal-difference update stays in PyTorch
 * (openkitchen_amd/dqn_cnn.py).  The rule is written out in include/okenv_qcnn.h (ok_qcnn_*); all matrix work runs on the f32-input
 * matrix cores.  The parameter vector is torch's parameters() order for the reference module (ok_qcnn_offsets); every weight must be
 * finite. */
typedef struct okenv_qcnn_config {
    int32_t  image_size;         /* S: 16 .. 128                                         (on this camera: 96)         */
    int32_t  kernel[3];          /* 1 .. 8                                               (8, 4, 3)                    */
    int32_t  stride[3];          /* 1 .. 4, at most the kernel                           (4, 2, 1)                    */
    int32_t  padding[3];         /* 0 .. 3, below the kernel                             (2, 1, 1)                    */
    int32_t  channels[3];        /* multiples of 16, 16 .. 128; ONE input channel        (32, 64, 64)                 */
    int32_t  hidden;             /* H: multiple of 16, 16 .. 512                         (512)                        */
    int32_t  num_actions;        /* A: 2 .. 8                                            (5)                          */
    int32_t  mode;               /* OKENV_ACTOR_GREEDY | OKENV_ACTOR_EPS_GREEDY                                       */
    float    epsilon;            /* [0, 1]; read by OKENV_ACTOR_EPS_GREEDY only                                       */
    uint32_t seed, agent_base;   /* key of the draws (okenv_actor_params'); global id of the handle's agent 0         */
    float    action_table[8][2]; /* (throttle_delta, steering_delta) per action index (DQCNNAgent::kActionMap); finite */
} okenv_qcnn_config;

/* What an act can leave behind for the caller, device pointers, each may be NULL */
typedef struct okenv_qcnn_record {
    float   *q;      /* [N][A] the Q-values                            */
    int64_t *action; /* [N]    the chosen index                        */
    float   *value;  /* [N]    q of the chosen action                  */
    uint8_t *alive;  /* [N]    1 where the agent was not crashed       */
} okenv_qcnn_record;

/* The frame ring's fields, capacity C: fp32 grey planes, what the learner's network consumes */
typedef struct okenv_qcnn_ring {
    float   *state;      /* [C][S][S] */
    float   *next_state; /* [C][S][S] */
    int64_t *action;     /* [C]       */
    float   *reward;     /* [C]       */
    float   *done;       /* [C] 1.0f or 0.0f */
} okenv_qcnn_ring;

/* Where okenv_qcnn_batch leaves a batch of B positions: each pointer may be NULL */
typedef struct okenv_qcnn_batch_out {
    float   *state;      /* [B][S][S] */
    float   *next_state; /* [B][S][S] */
    int64_t *action;     /* [B]       */
    float   *reward;     /* [B]       */
    float   *done;       /* [B]       */
    int32_t *index;      /* [B] the slot each position was read from */
} okenv_qcnn_batch_out;

#define OKENV_QCNN_BATCH_UNIFORM 0    /* slot ok_dqn_sample(seed, q, draw, size): the lidar ring's draw                        */
#define OKENV_QCNN_BATCH_SEQUENTIAL 1 /* push rank first + ((start + q) mod size): the reference's walk, wrapping at the end  */

/* LDS bytes of the larger of the two act kernels for the shape: a pure host function.  A shape is accepted only if this fits 160 KB.
 * 0 for a NULL config or a shape outside the rule's limits. */
OKENV_API int64_t okenv_qcnn_lds_bytes(const okenv_qcnn_config *config);
/* What names the kernels' paths for the shape: a pure host function.  plan [3]: the tiles of 16 hidden units a wave of the head kernel
 * owns (1 .. 4); what sizes the conv kernel's first LDS region (0: the grey plane inside its border, 1: layer 1's output inside its
 * border); whether the push and the gather move planes as 16-byte vectors (1: S S is a multiple of 4) or float by float (0). */
OKENV_API int okenv_qcnn_plan(const okenv_qcnn_config *config, int32_t *plan);
/* Attaches a Q-network to the handle (replaces an earlier one: its parameters are forgotten).  All device memory of the act is
 * allocated here.  OKENV_ERR_INVALID for NULL arguments, a shape outside the limits above or the LDS budget, an unknown mode, epsilon
 * outside [0, 1] or a non-finite entry of the action table. */
OKENV_API int okenv_qcnn_create(okenv_t h, const okenv_qcnn_config *config);
OKENV_API int okenv_qcnn_num_params(okenv_t h, int32_t *num_params);
/* New parameters from a host or device pointer (a device pointer is a device-to-device copy on the handle's stream); the kernels' own
 * copy of the weights is made behind it on the stream.  No synchronisation. */
OKENV_API int okenv_qcnn_set_params(okenv_t h, const float *params);
/* The parameters, in the same order, to a host or device pointer; synchronises. */
OKENV_API int okenv_qcnn_get_params(okenv_t h, float *params);
OKENV_API int okenv_qcnn_set_epsilon(okenv_t h, float epsilon);
/* A device word that is added to the draw index of every later okenv_qcnn_act (NULL: none); see okenv_actor_act. */
OKENV_API int okenv_qcnn_set_draw_offset(okenv_t h, const uint32_t *device_word);
/* Acts for every agent, crashed ones included, from frames (device, [N][S][S][4] uint8, frame_bytes = N S S 4 in all; 16-byte
 * aligned where S S is a multiple of 4, else 4-byte): writes OKENV_F_THROTTLE, OKENV_F_STEER and the record (rec may be NULL).  The
 * draw index and its device word are exactly okenv_actor_act's.  Two kernels on the handle's stream, no synchronisation, no
 * allocation: capturable beside okenv_step and okenv_render_views.  OKENV_ERR_STATE before okenv_qcnn_create or okenv_qcnn_set_params;
 * OKENV_ERR_INVALID for NULL frames or another frame_bytes. */
OKENV_API int okenv_qcnn_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_qcnn_record *rec);
/* okenv_qcnn_act's kernels one by one, for measurement: only those named in `stages`, in their order (the head reads what the conv
 * kernel left in the handle's buffer on an earlier call).  OKENV_QCNN_STAGE_HEAD_32 runs the head with 32 agents a workgroup instead of
 * the act's 16: the tiling that was measured and not chosen.  Refusals as okenv_qcnn_act's. */
#define OKENV_QCNN_STAGE_CONV 1u       /* grey, layers 0, 1 and 2 */
#define OKENV_QCNN_STAGE_HEAD 2u       /* fc1, fc2, the choice, the action fields and the record */
#define OKENV_QCNN_STAGE_HEAD_32 4u    /* the same with 32 agents a workgroup */
OKENV_API int okenv_debug_qcnn_stages(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_qcnn_record *rec, uint32_t stages);
/* Attaches the frame ring of `capacity` transitions (replaces an earlier one, whose memory is freed: a captured okenv_qcnn_push must
 * not be replayed afterwards).  flags: 0 or OKENV_REPLAY_PUSH_ALL.  OKENV_ERR_STATE before okenv_qcnn_create (the planes have the
 * network's size; a later okenv_qcnn_create with another image_size drops the ring).  Synchronises. */
OKENV_API int okenv_qcnn_ring_create(okenv_t h, int32_t capacity, uint32_t flags);
OKENV_API int okenv_qcnn_ring_reset(okenv_t h);
/* (transitions in the ring, transitions ever pushed); each pointer may be NULL; synchronises */
OKENV_API int okenv_qcnn_ring_size(okenv_t h, int64_t *size, int64_t *pushed);
/* The ring's fields, all `capacity` slots, to host or device pointers (each may be NULL); synchronises */
OKENV_API int okenv_qcnn_ring_get(okenv_t h, const okenv_qcnn_ring *out);
/* Appends the transitions of the step that has just run.  rec: what the preceding okenv_qcnn_act recorded (action; alive unless the
 * ring has OKENV_REPLAY_PUSH_ALL); frames: what that act saw; next_frames: the camera after the step; reward [N] on the device, or
 * NULL: the clearance rule (ok_dqn_reward).  Selection and rank are okenv_replay_push's.  Three kernels on the handle's stream, no
 * synchronisation, no allocation. */
OKENV_API int okenv_qcnn_push(okenv_t h, const okenv_qcnn_record *rec, const uint8_t *frames, const uint8_t *next_frames, int64_t frame_bytes,
                              const float *reward);
/* B positions of the ring into dense device arrays: mode OKENV_QCNN_BATCH_UNIFORM (start_or_draw: the draw index; the seed is the
 * config's) or _SEQUENTIAL (start_or_draw: the walk's start).  The ring's size is read on the device; an empty ring gives zeros.  One
 * kernel on the handle's stream, no synchronisation. */
OKENV_API int okenv_qcnn_batch(okenv_t h, int32_t B, int32_t mode, int64_t start_or_draw, const okenv_qcnn_batch_out *out);
/* The same rules on host arrays, no GPU needed.  act: frames [n][S][S][4]; crashed [n] or NULL; q [n][A], the others [n]; every
 * output may be NULL. */
OKENV_API int okenv_qcnn_act_host(const okenv_qcnn_config *config, const float *params, int32_t n, const uint8_t *frames, const uint8_t *crashed,
                                  uint32_t draw_index, float *throttle, float *steer, float *q, int64_t *action, float *value, uint8_t *alive);
/* One push on host arrays: ring [capacity] slots of image_size^2 planes and its counter; action, alive, crashed [n]; reward [n] or
 * NULL with dist [n][num_rays]. */
OKENV_API int okenv_qcnn_push_host(const okenv_qcnn_ring *ring, int32_t capacity, int32_t image_size, uint64_t *pushed, uint32_t flags, int32_t n,
                                   const int64_t *action, const uint8_t *alive, const uint8_t *frames, const uint8_t *next_frames,
                                   const uint8_t *crashed, const float *reward, const float *dist, int32_t num_rays);
OKENV_API int okenv_qcnn_batch_host(const okenv_qcnn_ring *ring, int32_t capacity, int32_t image_size, uint64_t pushed, uint32_t seed, int32_t B,
                                    int32_t mode, int64_t start_or_draw, const okenv_qcnn_batch_out *out);
/* Test hooks on host arrays: the grey planes [n][S][S] of frames [n][S][S][4]; and the network on grey planes [n][S][S] to q [n][A]
 * (the forward of okenv_qcnn_act_host behind its grey). */
OKENV_API int okenv_debug_qcnn_grey_host(int32_t image_size, int32_t n, const uint8_t *frames, float *planes);
OKENV_API int okenv_debug_qcnn_forward_planes_host(const okenv_qcnn_config *config, const float *params, int32_t n, const float *planes, float *q);

/* ---- Image transformer driver --------------------------------------------------------------------------------
 * DinoControl's frozen vision transformer (timm's vit_small_patch8_224.dino) and its 384-128-64-1 policy head, driven as
 * main_dino_control.cpp:80-89 drives them, for every agent of the handle: from the camera's RGBA8 frames (okenv_render_views, rendered
 * at image_size x image_size; the reference's bicubic resize is not part of the rule) the per-channel normalisation, the patch
 * embedding, the class token and positional table, `depth` pre-norm blocks (attention, GELU feed-forward), the final LayerNorm of the
 * class token and the head, to throttle_delta = throttle and steering_delta = clamp(output * steer_scale, +-steer_scale).  Inference
 * only.  The rule is written out in include/okenv_vit.h (ok_vit_*); all matrix work runs on the f32-input matrix cores.  The parameter
 * vector is torch's parameters() order of openkitchen_amd/dino.py's ViT (ok_vit_offsets); every weight must be finite. */
typedef struct okenv_vit_config {
    int32_t image_size;      /* S: a multiple of patch, (S / patch)^2 + 1 <= 1024 tokens   (the reference: 224)        */
    int32_t patch;           /* 4, 8 or 16                                                 (8)                         */
    int32_t dim;             /* D: multiple of 16, 16 .. 768                               (384)                       */
    int32_t heads;           /* dim / heads a multiple of 16, at most 64                   (6)                         */
    int32_t depth;           /* 1 .. 12                                                    (12)                        */
    int32_t dim_feedforward; /* multiple of 16, 16 .. 4 dim                                (1536)                      */
    int32_t head_hidden1;    /* multiples of 16, 16 .. 2048                                (128)                       */
    int32_t head_hidden2;    /*                                                            (64)                        */
    float   mean[3], std[3]; /* per channel, of pixel / 255; std > 0                       (ImageNet's)                */
    float   ln_eps;          /* inside every LayerNorm's root; > 0                         (1e-6)                      */
    float   throttle;        /* the constant throttle_delta; finite                        (100)                       */
    float   steer_scale;     /* steering_delta per unit of the output and its clamp; >= 0  (10)                        */
    int32_t agents_per_pass; /* agents whose activations the workspace holds; 0: as many as fit workspace_bytes, at least one */
    int64_t workspace_bytes; /* read when agents_per_pass is 0; 0: 1 GiB                                               */
} okenv_vit_config;

/* What an act can leave behind for the caller, device pointers, each may be NULL */
typedef struct okenv_vit_record {
    float   *action;    /* [N][2] throttle_delta, steering_delta                  */
    float   *output;    /* [N]    the head's output                               */
    float   *embedding; /* [N][D] the class token behind the final LayerNorm      */
    uint8_t *alive;     /* [N]    1 where the agent was not crashed               */
} okenv_vit_record;

/* LDS bytes of the largest of the act's kernels for the shape: a pure host function.  A shape is accepted only if this fits 160 KB.
 * 0 for a NULL config or a shape outside the rule's limits. */
OKENV_API int64_t okenv_vit_lds_bytes(const okenv_vit_config *config);
/* Attaches a policy to the handle (replaces an earlier one: its parameters are forgotten).  All device memory, the activations'
 * workspace included, is allocated here.  OKENV_ERR_INVALID for NULL arguments, a shape outside the limits above, an LDS plan
 * beyond 160 KB, a workspace beyond the kernels' index range or non-finite constants. */
OKENV_API int okenv_vit_create(okenv_t h, const okenv_vit_config *config);
OKENV_API int okenv_vit_num_params(okenv_t h, int32_t *num_params);
/* New parameters from a host or device pointer.  No synchronisation. */
OKENV_API int okenv_vit_set_params(okenv_t h, const float *params);
/* The parameters, in the same order, to a host or device pointer; synchronises. */
OKENV_API int okenv_vit_get_params(okenv_t h, float *params);
/* Acts for every agent, crashed ones included, from frames (device, 4-byte aligned, [N][S][S][4] uint8, frame_bytes = N S S 4 in
 * all): writes OKENV_F_THROTTLE, OKENV_F_STEER and the record (rec may be NULL).  A fixed sequence of 2 + 7 depth kernels per pass on
 * the handle's stream, no synchronisation, no allocation: capturable beside okenv_step and okenv_render_views.  OKENV_ERR_STATE before
 * okenv_vit_create or okenv_vit_set_params; OKENV_ERR_INVALID for NULL frames or another frame_bytes. */
OKENV_API int okenv_vit_act(okenv_t h, const uint8_t *frames, int64_t frame_bytes, const okenv_vit_record *rec);
/* The same rule on host arrays, no GPU needed: frames [n][S][S][4]; crashed [n] or NULL; every output may be NULL: throttle, steer,
 * output [n], embedding [n][D], alive [n]. */
OKENV_API int okenv_vit_act_host(const okenv_vit_config *config, const float *params, int32_t n, const uint8_t *frames, const uint8_t *crashed,
                                 float *throttle, float *steer, float *output, float *embedding, uint8_t *alive);
/* The attention piece alone (host pointers): qkv [seqs][T][3 heads dh] -> ctx [seqs][T][heads dh], on GPU `device` through the act's
 * own kernel; device < 0 (OKENV_DEBUG_ON_HOST) evaluates ok_vit_attend on the host.  1 <= T <= 1024, dh a multiple of 16 up to 64. */
OKENV_API int okenv_debug_vit_attend(int32_t device, int32_t seqs, int32_t T, int32_t heads, int32_t dh, const float *qkv, float *ctx);

/* ---- The image transformer driver's training: cached embeddings, head update -----------------------------------
 * DinoControl's recipe (train_dino_control.py): the backbone is frozen, so its embeddings are computed once (okenv_vit_embed) and the
 * head alone is trained on them with a weighted squared error against steering / steer_scale and Adam, one step per minibatch, in place
 * in the parameters okenv_vit_act reads.  The rule, with its summation order, is written out in include/okenv_vithead.h
 * (ok_vithead_*); every contraction of the update runs on the f32-input matrix cores. */

/* The frozen backbone over m frames (device, 4-byte aligned, [m][S][S][4] uint8, frame_bytes = m S S 4 in all; m is any positive
 * number, not the population): the final LayerNorm of every frame's class token to embedding [m][D] (device), bit for bit what
 * okenv_vit_act records.  Runs in passes of the act's agents_per_pass through the act's own workspace and kernels, and touches no
 * agent field.  No synchronisation, no allocation: capturable.  OKENV_ERR_STATE before okenv_vit_create or okenv_vit_set_params;
 * OKENV_ERR_INVALID for NULL arguments, m < 1 or another frame_bytes. */
OKENV_API int okenv_vit_embed(okenv_t h, const uint8_t *frames, int32_t m, int64_t frame_bytes, float *embedding);

typedef struct okenv_vit_head_params {
    float lr;        /* > 0                                        (the reference: 1e-4) */
    float beta1;     /* [0, 1), torch: 0.9                                               */
    float beta2;     /* [0, 1), torch: 0.999                                             */
    float eps;       /* > 0, torch: 1e-8                                                 */
    float weight;    /* of a sample whose |label| > threshold; > 0 (5)                   */
    float threshold; /* >= 0                                       (0.1)                 */
} okenv_vit_head_params;

/* The head's parameters [W1 | b1 | W2 | b2 | w3 | b3] (the tail of the driver's parameter vector) and Adam's moments, each
 * dim * hidden1 + hidden1 + hidden2 * hidden1 + hidden2 + hidden2 + 1 floats (57 601 at the reference shape); t: steps taken so far. */
typedef struct okenv_vit_head_state {
    float  *params, *m, *v;
    int64_t t;
} okenv_vit_head_state;

/* Where an update reports: device pointers (host pointers for okenv_vit_head_update_host), each may be NULL (skipped). */
typedef struct okenv_vit_head_output {
    float *loss; /* [epochs * ceil(M / B)]  per minibatch, from before its step         */
    float *grad; /* the last minibatch's gradient, in the head's parameter order        */
} okenv_vit_head_output;

/* LDS bytes of the update's forward kernel for a head dim -> hidden1 -> hidden2 -> 1: a pure host function.  A head is trained only
 * if this fits 160 KB.  0 for widths outside okenv_vit_config's limits. */
OKENV_API int64_t okenv_vit_head_lds_bytes(int32_t dim, int32_t hidden1, int32_t hidden2);
/* Attaches Adam state (m = v = 0, t = 0) for the head of the handle's policy; okenv_vit_create drops it again.  OKENV_ERR_STATE
 * before okenv_vit_create or okenv_vit_set_params; OKENV_ERR_INVALID for NULL arguments, lr <= 0, a beta outside [0, 1), eps <= 0,
 * weight <= 0, threshold < 0 (or NaN), a config whose steer_scale is 0, an LDS plan beyond 160 KB. */
OKENV_API int okenv_vit_head_learner_create(okenv_t h, const okenv_vit_head_params *params);
/* m = v = 0, t = 0 again.  (okenv_vit_set_params leaves the moments alone.) */
OKENV_API int okenv_vit_head_learner_reset(okenv_t h);
/* The head's parameters and Adam's moments to host or device pointers (each may be NULL), and t; synchronises. */
OKENV_API int okenv_vit_head_learner_get_state(okenv_t h, okenv_vit_head_state *out);
/* Enqueues every minibatch of every epoch on the handle's stream, two kernels each: no synchronisation, and no allocation after the
 * first call of a given min(B, M).  embedding [M][D], steer [M]: device; `order` is a device array [epochs][M] of int32 sample indices
 * or NULL (sequential).  Steps the head's slice of the handle's parameter vector in place: the next okenv_vit_act on the stream acts
 * with the new head and okenv_vit_get_params returns it.  The step number advances per enqueued minibatch.
 * OKENV_ERR_STATE before okenv_vit_head_learner_create; OKENV_ERR_INVALID for a NULL handle, embedding or steer, M, B or epochs < 1,
 * epochs * M >= 2^31. */
OKENV_API int okenv_vit_head_update(okenv_t h, const float *embedding, const float *steer, int32_t M, int32_t B, int32_t epochs, const int32_t *order,
                                    const okenv_vit_head_output *out);
/* The loss of every minibatch of one sequential pass with no update, to loss [ceil(M / B)] (device): the validation loop. */
OKENV_API int okenv_vit_head_eval(okenv_t h, const float *embedding, const float *steer, int32_t M, int32_t B, float *loss);
/* The same rule on host arrays, no GPU needed.  okenv_vit_act_host gives the embedding on the host. */
OKENV_API int okenv_vit_head_update_host(const okenv_vit_head_params *params, int32_t dim, int32_t hidden1, int32_t hidden2, float steer_scale,
                                         okenv_vit_head_state *state, const float *embedding, const float *steer, int32_t M, int32_t B, int32_t epochs,
                                         const int32_t *order, const okenv_vit_head_output *out);
OKENV_API int okenv_vit_head_eval_host(const okenv_vit_head_params *params, int32_t dim, int32_t hidden1, int32_t hidden2, float steer_scale,
                                       const float *head, const float *embedding, const float *steer, int32_t M, int32_t B, float *loss);

/* ---- zero-copy access for device-side callers ------------------------ */

/* Device address and size of one library-owned struct-of-arrays field (okenv_field), valid for the handle's lifetime.
 * Work on it must be ordered against the handle's stream (okenv_set_stream / okenv_sync).  This is what the batched
 * Python binding wraps into tensors instead of copying sensor_hits_ / crashed_ out per step the way
 * Pybind/bindings.cpp:36-52 round-trips one agent. */
OKENV_API int okenv_field_device_ptr(okenv_t h, int32_t field, void **ptr, uint64_t *bytes);

/* Agent::sensor_hits_ as interleaved (x,y) pairs [N*R*2], Agent::sensor_hits_[r].norm() [N*R], and
 * crashed_/timed_out_ as bit0/bit1 of one byte per agent.  Synchronise. */
OKENV_API int okenv_get_hits(okenv_t h, float *out_xy);
OKENV_API int okenv_get_distances(okenv_t h, float *out);
OKENV_API int okenv_get_flags(okenv_t h, uint8_t *out);

/* ---- packed host exchange for callers that keep Agent objects on the host (the C++ facade) -------------------- */

/* One agent's mutable state as a record: the population crosses PCIe in ONE copy each way per step instead of one
 * copy per field (Environment::step of the facade was 40 small copies = 370 us for a single agent before this). */
typedef struct okenv_agent_record {
    float    pos_x, pos_y, rot, speed, acc, throttle, steer; /* Agent::pos_, rot_, speed_, acceleration_, current_action_ */
    float    disp_x, disp_y;                                 /* DisplacementStats::init_pos                              */
    uint32_t disp_ctr;                                       /* DisplacementStats::displacement_ctr                      */
    uint8_t  mode, crashed, timed_out, disp_timed_out;       /* movement_mode_, crashed_, timed_out_, displacement_timed_out */
} okenv_agent_record;                                        /* 44 bytes */

#define OKENV_PACKED_WITH_STATS 1u   /* the DisplacementStats members travel too (Environment::step); otherwise the   */
                                     /* device keeps its own and the record's are left untouched                     */
#define OKENV_PACKED_COLLIDE_ONLY 2u /* CollisionChecker::checkCollision(): no kinematics, no standstill bookkeeping  */
/* Upload `in[num_agents]`, run one Environment::step (or only the collision pass), download the new state into
 * `out[num_agents]` (may alias `in`) and Agent::sensor_hits_ as interleaved (x, y) pairs into sensor_hits_xy
 * [num_agents * num_rays * 2].  Host pointers; synchronises.
 * Up to 64 single-wave agents, OKENV_PACKED_WITH_STATS steps: when such calls follow each other within 100 us, a
 * resident step kernel takes them over (no launch per step; okenv_info.packed_resident).  It leaves after 300 us
 * without a step and before any other call on the handle does its work; results are the same bits either way.
 * Environment variable OKENV_RESIDENT: 0 = never, 1 = from the first eligible call on. */
OKENV_API int okenv_step_packed(okenv_t h, const okenv_agent_record *in, okenv_agent_record *out, float *sensor_hits_xy,
                                uint32_t flags);

/* ---- the hot path -------------------------------------------------------------------------------- */

/* Environment::step() x n_steps (Environment/Environment.cpp:125-149, minus render): move + standstill for
 * non-crashed agents, then the collision pass for all.  Uses the actions currently stored. */
OKENV_API int okenv_step(okenv_t h, int32_t n_steps);
/* CollisionChecker::checkCollision() alone (Environment/CollisionChecker.cu:197-200): ray build, first-hit
 * raycast, hit transform, crash flag; no kinematics. */
OKENV_API int okenv_collide(okenv_t h);
/* The bench driver loop on the device (shape of RLRacers/GuidedCostLearning/test.cpp:100-117; recipe in
 * SURVEY.md section 8d): per step, crashed agents are re-placed on a Philox-chosen centre-line point, every
 * agent draws throttle~U[0,100) and steer~U[-5,5) from Philox4x32 keyed (seed; agent_base+i, step_base+s),
 * then Environment::step.  Requires okenv_set_centerline. */
OKENV_API int okenv_rollout_random(okenv_t h, int32_t n_steps, uint32_t seed, uint32_t agent_base, uint32_t step_base);
/* Bench initial state: agent i on centre-line index ((agent_base+i)*2654435761 mod 2^32) mod P with the track
 * heading, speed 0, DisplacementStats and hit points zeroed, all agents in `mode`. */
OKENV_API int okenv_init_bench_state(okenv_t h, uint32_t agent_base, int32_t mode);
/* RaceTrack::findNearestTrackIndexBruteForce (Environment/RaceTrack.cpp:16-31) for n query points
 * (host or device pointers), or for every agent's current position when qx == NULL (n ignored). */
OKENV_API int okenv_nearest_track_idx(okenv_t h, const float *qx, const float *qy, int32_t n, int32_t *out);

/* ---- EvolutionaryRacer on the device (BASELINE configs 3 and 4) --------- */

/* genetic::Network() for every agent (EvolutionaryRacer/Network.hpp:99-107): (R+2) -> hidden -> 6, no biases, weights
 * U[-1,1) from Philox keyed (seed; agent_base+i, weight) in place of the unseeded Eigen Random().  hidden <= 32
 * (30 in the reference).  Needs 5 <= R <= 64.  Weights live on the device, okenv_policy_mlp_weights_per_agent()
 * floats per agent in the padded layout of include/okenv_math.h. */
OKENV_API int okenv_policy_mlp_create(okenv_t h, int32_t hidden, uint32_t seed, uint32_t agent_base);
OKENV_API int32_t okenv_policy_mlp_weights_per_agent(okenv_t h);
OKENV_API int okenv_policy_mlp_get_weights(okenv_t h, float *out);       /* host or device pointer */
OKENV_API int okenv_policy_mlp_set_weights(okenv_t h, const float *in);  /* host or device pointer */
/* n_steps x { GeneticAgent::updateAction for every agent (GeneticAgent.hpp:37-107, Network::infer Network.hpp:119-155)
 * from the previous step's observation; Environment::step } -- the inner loop of genetic_learner_sim.cpp:76-95, fused
 * into the step kernel.  Call okenv_step(h, 1) once after a reset for the initial observation (:75). */
OKENV_API int okenv_rollout_policy(okenv_t h, int32_t n_steps);
/* number of agents with crashed_ == false (the loop's all_done test, genetic_learner_sim.cpp:85-92) */
OKENV_API int okenv_alive_count(okenv_t h, int32_t *out);

/* ---- episodes: "step everybody until every agent has crashed" ----------------------------------------------------
 * The inner loop of both population callers (EvolutionaryRacer/genetic_learner_sim.cpp:76-95,
 * RLRacers/Q_Learning/q_racer_sim.cpp:156-190) runs until the step T in which the LAST agent crashes; most agents crash
 * long before that (a tenth to a fifth of the agent-steps of such a loop belong to agents still alive).  Between
 * okenv_episode_begin and okenv_episode_end the policy rollouts (okenv_rollout_policy, okenv_rollout_q) therefore
 *   - step only the agents that can still change: after an agent's first step as a crashed agent nothing about it changes
 *     any more (it does not move, its standstill counter does not tick, its rays keep their stale hit points, the MLP policy
 *     sees the same inputs), so it is dropped -- by a wave of the running launch as soon as all its agents are done, and from
 *     the launch grid by okenv_episode_compact;
 *   - may overrun T (launches end where the caller's n_steps end): okenv_episode_end finds T and leaves every agent, every
 *     Q table and the step count exactly as the reference's loop leaves them after step T, whatever the launches' lengths.
 *     Q-learning's per-step update of CRASHED agents (epsilon-greedy draw + learn with reward -200, q_racer_sim.cpp:158-182)
 *     is replayed per agent for its steps crash+1 .. T at that point.
 * Typical loop:   okenv_episode_begin(h);  okenv_episode_tail_limit(h, &tail);  listed = N;
 *                 do { okenv_rollout_policy(h, listed <= tail ? all the steps still allowed : n);
 *                      okenv_episode_compact(h, &alive, &listed); } while (alive > 0 && more steps allowed);
 *                 okenv_episode_end(h, &steps, &live);
 * Needs auto-reset off.  Any call that changes agent state from outside (set/upload/reset/step without a policy) ends the
 * episode without the end-of-episode corrections.  While a controller episode is running (okenv_rollout_controller inside
 * okenv_episode_begin / _end) okenv_tracker_begin, okenv_tracker_update and okenv_controller_set_params return OKENV_ERR_STATE:
 * the fused rollout carries the bookkeeping itself.  A population no larger than okenv_episode_tail_limit is listed from
 * okenv_episode_begin on (its first rollout already runs one agent per workgroup). */
OKENV_API int okenv_episode_begin(okenv_t h);
/* Rebuilds the list of agents the next rollouts step; *alive_out = agents with crashed_ == false (the loop's all_done test),
 * *listed_out = agents still stepped (alive ones + those that crashed in the last step taken).  Either may be NULL. */
OKENV_API int okenv_episode_compact(okenv_t h, int32_t *alive_out, int32_t *listed_out);
/* Longest list (okenv_episode_compact's *listed_out) that is stepped one agent per workgroup on this handle (0: never).  Such
 * a workgroup leaves as soon as its agent is done, so from there on the caller may ask for ALL the steps it still allows in
 * one rollout call: the launch ends with the step in which the last agent crashes, and no launch boundary is paid any more. */
OKENV_API int okenv_episode_tail_limit(okenv_t h, int32_t *out);
/* *steps_out = T (steps of the reference's loop; all steps taken if somebody is still alive), *live_agent_steps_out = sum over
 * the steps of the agents that entered the step alive.  Either may be NULL. */
OKENV_API int okenv_episode_end(okenv_t h, int32_t *steps_out, uint64_t *live_agent_steps_out);
/* Agents whose position lies outside the raycast grid's box (the track's bounding box plus a small pad): *alive_off_grid those
 * with crashed_ == false, *all_off_grid all of them (either may be NULL).  The crash test is lidar-only and a step can be 1.6 px
 * long, so an agent can tunnel through both boundary polylines (Environment/CollisionChecker.cu:167-171);
 * outside, nothing is within sensor range and only the standstill timeout (Environment.cpp:16-39) can still end it -- at speed it
 * never does, and "until every agent has crashed" then runs into the caller's step cap.  Measurement aid; synchronises. */
OKENV_API int okenv_off_grid_count(okenv_t h, int32_t *alive_off_grid, int32_t *all_off_grid);
/* Agent::reset of EVERY agent to one pose (genetic_learner_sim.cpp:65-70) */
OKENV_API int okenv_reset_all(okenv_t h, float x, float y, float rot_deg);
/* assignScores (EvolutionaryRacer/MiscUtils.hpp:64-71): score = nearest centre-line index as float, kept on the
 * device for okenv_ga_select_mate; `out` (N floats, host or device) may be NULL. */
OKENV_API int okenv_ga_scores(okenv_t h, float *out);
/* Where that score vector lives: the device address of the N floats okenv_ga_scores fills (library-owned, valid for the
 * handle's lifetime), and the hipStream_t the handle enqueues its work on.  With the two a multi-GPU caller runs its one
 * collective -- the per-generation all-gather of this vector, SURVEY.md section 8e -- straight from device memory and in
 * stream order behind the kernel that wrote it:  okenv_ga_scores(h, NULL); ncclAllGather(scores, colony, N, ncclFloat, comm,
 * stream);  (openkitchen_amd/csrc/apps/genetic_learner_sim.cpp --gpus N). */
OKENV_API int okenv_ga_scores_device(okenv_t h, const float **ptr);
OKENV_API int okenv_get_stream(okenv_t h, void **hip_stream);
/* chooseAndMateAgents (EvolutionaryRacer/Mating.hpp:108-166) with mate2AgentsSelective (:52-99): the 5 best agents
 * (ties to the lower index) become parents; offspring 0 clones the best, offspring 1 is the best mated with itself,
 * every other offspring draws two different parents proportionally to score; per weight 10 % mutation to U[-1,1),
 * else the dominant parent's weight with probability 0.75.  Draws come from Philox keyed (seed; agent_base+offspring,
 * weight, generation) instead of std::random_device.  parents_out (5 ints, host) may be NULL. */
OKENV_API int okenv_ga_select_mate(okenv_t h, uint32_t seed, uint32_t generation, uint32_t agent_base, int32_t *parents_out);

/* ---- RLRacers/Q_Learning on the device (BASELINE config 5) ----------------------- */

/* One 243 x 3 table per agent, every entry numeric_limits<float>::lowest() (RLRacers/Q_Learning/QAgent.hpp:31-36,64-68).
 * The state uses five rays; with a fan of more than five rays the ones nearest to -70, -30, 0, +30, +70 degrees are taken
 * (ties to the lower index) -- the reference fan is exactly those five (QAgent.hpp:56-62).  Needs R >= 5 and the LDS form. */
OKENV_API int okenv_q_create(okenv_t h);
/* Start of an episode (q_racer_sim.cpp:129-154): every agent reset onto centre-line point `reset_idx` with the track
 * heading, prev_track_idx = that point's nearest index, one Environment::step for the initial observation, current
 * state = discretizeState().  All agents must be in VELOCITY mode (the action map sets the speed). */
OKENV_API int okenv_q_begin_episode(okenv_t h, int32_t reset_idx);
/* n_steps x { updateAction (epsilon-greedy, QAgent.hpp:98-119); Environment::step; discretizeState; reward
 * (QAgent.hpp:150-168, nearest centre-line index); learn (QAgent.hpp:121-138) } for every agent, crashed ones included, as
 * q_racer_sim.cpp:158-182 does.  Random draws: Philox keyed (seed; agent_base+i, step_base+s).  Inside an episode
 * (okenv_episode_begin) the crashed agents' share of this is deferred to okenv_episode_end, with the same result; epsilon,
 * seed and agent_base must then stay the same for the whole episode and step_base advance with the steps taken. */
OKENV_API int okenv_rollout_q(okenv_t h, int32_t n_steps, float epsilon, uint32_t seed, uint32_t agent_base, uint32_t step_base);
OKENV_API int okenv_q_get_table(okenv_t h, float *out);      /* [N][243][3], host or device pointer */
OKENV_API int okenv_q_set_table(okenv_t h, const float *in);
/* current_state_idx_, current_action_idx_, prev_track_idx_ per agent (host arrays, any may be NULL) */
OKENV_API int okenv_q_get_state(okenv_t h, int32_t *state, int32_t *action, int32_t *prev_idx);

/* shareCumulativeKnowledge (q_racer_sim.cpp:24-75; off by default in the reference, :16): `okenv_q_table_sums` gives, per
 * (state, action), the sum of the valid entries over this handle's agents and their count (729 floats each, host or
 * device pointers); `okenv_q_assign_mean` sets every agent's table to sum/count (entries with count 0 stay invalid).  A
 * multi-GPU caller all-reduces the two vectors between the calls (5.8 KB); `okenv_q_share_knowledge` does both locally. */
OKENV_API int okenv_q_table_sums(okenv_t h, float *sum, float *count);
OKENV_API int okenv_q_assign_mean(okenv_t h, const float *sum, const float *count);
OKENV_API int okenv_q_share_knowledge(okenv_t h);

/* ---- bird's-eye camera views of every agent ----------------------------------------------------
 * The frame the reference's image-based applications pull from the window every step (Visualizer::render with the camera
 * following one agent at zoom 15, Environment/Visualizer.cpp:75-80,159-223, read back by ScreenGrabber::getRenderTargetDevice
 * and flipped), rendered for ALL N agents at once by one kernel into a device buffer.  The rule, exactly (it is our own; raylib's
 * rasteriser bits are not claimed):
 *
 * Geometry: the reference's draw list, six shadeAreaBetweenCurves calls (Visualizer.cpp:99-138,176-194): ordinal 0 right_bound_inner_ /
 *   right_bound_outer_ (blue 0,0,255), 1 left_bound_inner_ / left_bound_outer_ (red 255,0,0), 2 left_bound_inner_ / right_bound_inner_
 *   (green 0,255,0), 3 start_line_ / finish_line_ = {ro.front, ro.back} / {lo.front, lo.back} (green), 4 {ri.front, ri.back} /
 *   {ro.front, ro.back} (blue), 5 {li.front, li.back} / {lo.front, lo.back} (red): 6P triangles, each in the vertex order the
 *   reference hands to DrawTriangle after its cross-product reorder (okenv_track_band_triangles lists them).
 * Inside test, fp32 without contraction, for a triangle (a, b, c) and a sample p: e0 = (b.x-a.x)*(p.y-a.y) - (b.y-a.y)*(p.x-a.x),
 *   e1 and e2 the same for the edges (b, c) and (c, a); inside iff all three >= 0 or all three <= 0.  A triangle whose
 *   area (b.x-a.x)*(c.y-a.y) - (b.y-a.y)*(c.x-a.x) is exactly 0 covers nothing.  A sample's band is the LARGEST ordinal among the
 *   triangles containing it (later draws paint over earlier ones); none: background (0,0,0).
 * Camera: step_x = view_w / (width*samples), half_x = view_w * 0.5f (fp32, host; y alike).  Sample column col = u*samples + j:
 *   ox = ((float)col + 0.5f) * step_x - half_x; oy from the row alike.  Row 0 is the smallest world y (the frame after the
 *   applications' flip({0})).  World-aligned (the reference's camera): wx = pos_x + ox, wy = pos_y + oy.  OKENV_VIEW_HEADING_UP:
 *   (cs, sn) = cos, sin of OK_DEG2RAD * rot from ok_sincosf, wx = pos_x + (ox*(-sn) - oy*cs), wy = pos_y + (ox*cs - oy*sn).
 * Agent (drawAgent, Visualizer.cpp:48-64; only the view's own agent): dx = wx - pos_x, dy = wy - pos_y; in the disc iff
 *   dx*dx + dy*dy <= radius*radius; with OKENV_VIEW_DRAW_HEADING, in the white heading half iff dx*cs + dy*sn >= 0.  The disc has
 *   the agent colour, or if crashed_ (253,249,0) at alpha 150 over the band: (253*150 + under*105 + 127) / 255 per channel.
 * Formats, destination contiguous [N, H, W, C] uint8: OKENV_VIEW_RGBA8 (C = 4, alpha 255; samples > 1: per channel the box filter
 *   (sum + s*s/2) / (s*s) over the s*s samples -- the applications' bilinear resize of a 1600x1400 frame differs from it at
 *   edges), OKENV_VIEW_CLASS8 (C = 1, samples 1 only): 0 background, 1 right shoulder (ordinals 0, 4), 2 left shoulder (1, 5),
 *   3 driving surface (2, 3), 4 agent, 5 heading half, 6 crashed agent.
 */
#define OKENV_VIEW_RGBA8 0
#define OKENV_VIEW_CLASS8 1
#define OKENV_VIEW_DRAW_AGENT 1u
#define OKENV_VIEW_DRAW_HEADING 2u
#define OKENV_VIEW_HEADING_UP 4u
/* the reference's follow camera: a 1600 x 1400 window at zoom 15 (Visualizer.cpp:75-80) */
#define OKENV_VIEW_FOLLOW_W (1600.0f / 15.0f)
#define OKENV_VIEW_FOLLOW_H (1400.0f / 15.0f)

typedef struct okenv_view_desc {
    int32_t  width, height;   /* output pixels, 1..1024 each                                                  */
    int32_t  samples;         /* per axis: 1, 2 or 4                                                          */
    int32_t  format;          /* OKENV_VIEW_RGBA8 / OKENV_VIEW_CLASS8                                         */
    float    view_w, view_h;  /* world extent [px], finite and > 0 (OKENV_VIEW_FOLLOW_W / _H)                  */
    uint32_t flags;           /* OKENV_VIEW_DRAW_AGENT | OKENV_VIEW_DRAW_HEADING | OKENV_VIEW_HEADING_UP      */
    float    radius;          /* Agent::radius_ (Agent.h:60: 9), finite and > 0                               */
    uint8_t  agent_rgb[3];    /* Agent::color_ (Agent.h:63: 80, 80, 80)                                       */
    uint8_t  reserved;
} okenv_view_desc;

typedef struct okenv_render_info {
    int32_t  triangles;       /* of the draw list, zero-area ones left out                                    */
    int32_t  grid_nx, grid_ny;
    float    grid_cell;       /* cell edge [px]                                                               */
    int32_t  registrations;   /* triangle copies over all cells                                               */
    int32_t  solid_cells;     /* cells whose samples skip the tests (0: not used)                             */
    int32_t  width, height, samples, channels;
    uint64_t bytes_per_call;  /* N * H * W * C                                                                */
} okenv_render_info;

/* Builds the draw list from the four boundary polylines (xy pairs, num_points >= 2 each, host pointers), its grid, and uploads
 * them; replaces an earlier render setup of the handle.  Synchronises. */
OKENV_API int okenv_render_create(okenv_t h, const float *left_inner_xy, const float *left_outer_xy, const float *right_inner_xy,
                                  const float *right_outer_xy, int32_t num_points, const okenv_view_desc *desc);
/* Renders every agent's view into `dst` (device memory of the handle's device, >= N*H*W*C bytes) from the current pos_x, pos_y,
 * rot, crashed_ (read only).  One kernel on the handle's stream, no synchronisation: it can be captured into a HIP graph next to
 * okenv_step.  OKENV_ERR_STATE before okenv_render_create. */
OKENV_API int okenv_render_views(okenv_t h, void *dst, uint64_t dst_bytes);
OKENV_API int okenv_render_get_info(okenv_t h, okenv_render_info *out);
/* The draw list of a track (host only, no GPU): 6P triangles as (a.x, a.y, b.x, b.y, c.x, c.y) in DrawTriangle's order and their
 * draw ordinals; returns the count (6P), or < 0 on error, and writes min(count, cap) entries (either output may be NULL). */
OKENV_API int okenv_track_band_triangles(okenv_track_t t, float *xy6, uint8_t *ordinal, int32_t cap);

/* ---- measurement --------------------------------------------------------------------------------- */

/* When enabled, every step/collide/rollout launch is bracketed by HIP events on the handle's stream. */
OKENV_API int okenv_set_timing(okenv_t h, int32_t enabled);
/* Sum of the bracketed kernel durations [ms] and their count since the last call; synchronises, then clears. */
OKENV_API int okenv_get_timing(okenv_t h, double *total_ms, uint64_t *launches);

/* ---- host-side track construction (RaceTrack + TrackSegments, no GPU involved) -------------------- */

/* RaceTrack::RaceTrack(csv) (Environment/RaceTrack.cpp:3-14). */
OKENV_API int okenv_track_load(okenv_track_t *out, const char *csv_path);
OKENV_API int okenv_track_free(okenv_track_t t);
OKENV_API int32_t okenv_track_num_points(okenv_track_t t);
OKENV_API int32_t okenv_track_num_segments(okenv_track_t t);
/* which: 0 x_m, 1 y_m, 2 w_tr_right_m, 3 w_tr_left_m, 4 headings_ (P floats);
 *        5 left_bound_inner_, 6 left_bound_outer_, 7 right_bound_inner_, 8 right_bound_outer_ (2P floats, xy) */
OKENV_API int okenv_track_get(okenv_track_t t, int32_t which, float *out);
/* RaceTrack::getNearestDistanceToTrackBoundary and RaceTrack::getDistanceToLaneCenter (Environment/RaceTrack.h:36,39,
 * RaceTrack.cpp:33-72) for n query points (host pointers; either output may be NULL).  Host-side, like the reference's. */
OKENV_API int okenv_track_queries(okenv_track_t t, const float *qx, const float *qy, int32_t n, float *out_boundary_distance,
                                  float *out_lane_center_ratio);
/* TrackSegments::TrackSegments (Environment/TrackSegments.cu:6-42): 4*P segments, x1,y1,x2,y2 each. */
OKENV_API int okenv_track_segments(okenv_track_t t, float *out_xyxy);

/* Work the broad phase leaves for the population's current poses (measurement aid: SURVEY.md section 8d's S_tested): every
 * live agent's rays walked once through the grid; out[0] = rays, out[1] = exact ray-segment tests (the reference's sweep,
 * Environment/CollisionChecker.cu:49-67, makes num_segments per ray), out[2] = grid cells entered, out[3] = boundary points
 * evaluated by the skip rule.  LDS form of the grid only. */
OKENV_API int okenv_work_stats(okenv_t h, uint64_t out[4]);
/* The same walk as the step kernels make it with the front / back split of the segment set (okenv_info.front_back_bytes > 0;
 * openkitchen_amd/csrc/ok_grid.h: the outer boundary polylines sit in an image of their own and are walked only by rays whose
 * origin is not certified to lie between the inner boundaries, or whose front walk may have missed a crossing): out[0..3] as
 * above, front and back walks together; out[4] rays of a certified origin, out[5] rays whose front walk was ambiguous, out[6] rays
 * that walked the back image too; out[7] unused.  OKENV_ERR_STATE when the segment set has no split. */
OKENV_API int okenv_work_stats_split(okenv_t h, uint64_t out[8]);

/* ---- device self-checks used by the parity tests --------------------------------------------------- */

/* ok_atan2f (include/okenv_math.h) and the experts' bounded normalizeAngleDeg on host arrays; host only, no GPU. */
OKENV_API int okenv_debug_atan2f(const float *y, const float *x, float *out, int32_t n);
OKENV_API int okenv_debug_expert_normalize_angle(const float *angle_deg, float *out, int32_t n);
/* ok_expf (the actors' softmax) on a host array; host only, no GPU. */
OKENV_API int okenv_debug_expf(const float *x, float *out, int32_t n);
/* ok_logf of okenv_math.h for n positive finite arguments (host evaluation) */
OKENV_API int okenv_debug_logf(const float *x, float *out, int32_t n);
/* REINFORCE's dropout mask of hidden units 0 .. hidden-1 for (p, seed, global agent id, draw index): 1 kept, 0 dropped (host) */
OKENV_API int okenv_debug_reinforce_mask(float p, uint32_t seed, uint32_t agent, uint32_t draw, int32_t hidden, uint8_t *out);
/* Device milliseconds of the five kernels of the handle's latest okenv_batch_prepare (walk, tree, count, scan, gather), from events
 * it records between them while okenv_set_timing is on; waits for the last one.  OKENV_ERR_STATE when that call ran untimed. */
OKENV_API int okenv_debug_batch_timing(okenv_t h, double *ms5);
/* Device milliseconds of the handle's latest okenv_ppo_update, summed over its minibatches per kernel (gradient partials, join +
 * Adam), from events it records between them while okenv_set_timing is on; waits for the last one.  OKENV_ERR_STATE when that call
 * ran untimed. */
OKENV_API int okenv_debug_update_timing(okenv_t h, double *ms2);
/* The same for the handle's latest okenv_dqn_update, summed over its iterations per kernel (gradient partials, join + Adam). */
OKENV_API int okenv_debug_dqn_timing(okenv_t h, double *ms2);
/* The same for the handle's latest okenv_ddpg_update: critic gradient, critic step, actor gradient, actor step. */
OKENV_API int okenv_debug_ddpg_timing(okenv_t h, double *ms4);
/* of the latest okenv_reinforce_update likewise: [0] gradient kernels, [1] join kernels (accumulate and Adam), summed over the slices */
OKENV_API int okenv_debug_reinforce_timing(okenv_t h, double *ms2);
/* of the latest okenv_gauss_update likewise: [0] gradient kernels, [1] join kernels */
OKENV_API int okenv_debug_gauss_timing(okenv_t h, double *ms2);
/* of the latest okenv_gcl_cost_update (which = OKENV_GCL_COST) or of network `which`'s slices in the latest okenv_gcl_policy_update
 * likewise: [0] gradient kernels, [1] join kernels */
OKENV_API int okenv_debug_gcl_timing(okenv_t h, int32_t which, double *ms2);
/* ok_gauss_normal_pair (include/okenv_gauss.h) on n word pairs (host pointers): out0 = r cos, out1 = r sin; on GPU `device`, or on the
 * host with device == OKENV_DEBUG_ON_HOST. */
OKENV_API int okenv_debug_normal(int32_t device, const uint32_t *w0, const uint32_t *w1, float *out0, float *out1, int32_t n);
/* ok_learn_adam (include/okenv_learn.h) on host arrays: step number t >= 1 of n parameters p with moments m, v and gradients g, all
 * updated in place; host only, no GPU. */
OKENV_API int okenv_debug_adam(const okenv_learner_params *params, int64_t t, float *p, float *m, float *v, const float *g, int32_t n);
/* ok_sincosf evaluated on the GPU (n values, host pointers). */
OKENV_API int okenv_debug_sincos(int32_t device, const float *x, float *s, float *c, int32_t n);
/* One leaf function of include/okenv_math.h on n values (host pointers), evaluated on GPU `device` by one elementwise kernel, or,
 * with device == OKENV_DEBUG_ON_HOST, by the host compilation of the same header inside the library (no GPU needed).  The two must
 * agree bit for bit: tests/test_gpu_math.py runs both over the whole argument range.  `b` is read by OKENV_FN_ATAN2 only (a = y,
 * b = x) and OKENV_FN_SINCOS_PAIR; `out1` is written by OKENV_FN_SINCOS (out0 = sine, out1 = cosine) and OKENV_FN_SINCOS_PAIR only;
 * both may be NULL otherwise. */
enum okenv_debug_fn {
    OKENV_FN_SINCOS,                 /* ok_sincosf */
    OKENV_FN_TANH,                   /* ok_tanhf */
    OKENV_FN_EXP,                    /* ok_expf */
    OKENV_FN_LOG,                    /* ok_logf */
    OKENV_FN_ATAN2,                  /* ok_atan2f(a, b) */
    OKENV_FN_NORMALIZE_ANGLE,        /* ok_normalize_angle_deg */
    OKENV_FN_EXPERT_NORMALIZE_ANGLE, /* ok_expert_normalize_angle_deg */
    OKENV_FN_SINCOS_PAIR,            /* ok_sincosf_pair(a, b): out0 and out1 hold 2 n floats, the sine and cosine of a[i] in
                                        out0[2 i], out0[2 i + 1], those of b[i] in out1[2 i], out1[2 i + 1] */
    OKENV_FN_ERF,                    /* ok_erff */
    OKENV_NUM_DEBUG_FNS
};
#define OKENV_DEBUG_ON_HOST (-1)
OKENV_API int okenv_debug_math(int32_t device, int32_t fn, const float *a, const float *b, float *out0, float *out1, int32_t n);
/* okenv_debug_adam with ok_learn_adam evaluated per element on GPU `device` (ok_learn_factors on the host, as in every learner); the
 * arrays are host pointers and are updated in place.  device == OKENV_DEBUG_ON_HOST evaluates on the host.  Unlike the learners'
 * entries this one accepts eps == 0, so that the division's zero and infinite denominators can be compared too. */
OKENV_API int okenv_debug_adam_device(int32_t device, const okenv_learner_params *params, int64_t t, float *p, float *m, float *v, const float *g,
                                      int32_t n);
/* First-hit parameter t for n arbitrary rays (origin, angle [rad]) through the handle's grid (host pointers). */
OKENV_API int okenv_debug_cast_rays(okenv_t h, const float *ox, const float *oy, const float *angle_rad, int32_t n, float *out_t);

/* The step-kernel launches of openkitchen_amd/csrc/okenv_capi.hip (the cases of launchStep), one per instantiation the
 * launcher can pick.  The tests use them to check which form a call ran. */
enum okenv_step_form {
    OKENV_FORM_TAIL_Q,             /* okStepTailKernel<kPolicyQ, 0>: a short Q-learning episode list, one agent per workgroup */
    OKENV_FORM_TAIL_MLP32,         /* okStepTailKernel<kPolicyMlp, 32> */
    OKENV_FORM_TAIL_MLP15,         /* okStepTailKernel<kPolicyMlp, 15> */
    OKENV_FORM_TAIL_MLP,           /* okStepTailKernel<kPolicyMlp, 0>: any other fan */
    OKENV_FORM_COOP_Q,             /* okStepCoopKernel<kPolicyQ> */
    OKENV_FORM_COOP_CTRL,          /* okStepCoopKernel<kPolicyCtrl> */
    OKENV_FORM_COOP_MLP32,         /* okStepCoopKernel<kPolicyMlp, false, false, false, 32>: 32 rays in 32-lane groups */
    OKENV_FORM_COOP_MLP,           /* okStepCoopKernel<kPolicyMlp> */
    OKENV_FORM_COOP_PACKED_DIRECT, /* okStepCoopKernel<kPolicyNone, true, false, true>: okenv_step_packed, direct intervals */
    OKENV_FORM_COOP_PACKED,        /* okStepCoopKernel<kPolicyNone, true> */
    OKENV_FORM_COOP_DIRECT,        /* okStepCoopKernel<kPolicyNone, false, false, true> */
    OKENV_FORM_COOP_G64_RANDOM,    /* okStepCoopKernel<kPolicyNone, false, false, false, 64, true>: okenv_rollout_random */
    OKENV_FORM_COOP_G64,           /* okStepCoopKernel<kPolicyNone, false, false, false, 64> */
    OKENV_FORM_COOP,               /* okStepCoopKernel<kPolicyNone> */
    OKENV_FORM_RESIDENT_DIRECT,    /* okStepCoopKernel<kPolicyNone, true, true, true>: the resident packed step */
    OKENV_FORM_RESIDENT,           /* okStepCoopKernel<kPolicyNone, true, true> */
    OKENV_FORM_LDS,                /* okStepKernel<kGridLds, kPolicyNone>: every lane walks its own rays (OKENV_COOP=0, or > 64 rays) */
    OKENV_FORM_LDS_MLP,            /* okStepKernel<kGridLds, kPolicyMlp> */
    OKENV_FORM_GLOBAL,             /* okStepKernel<kGridGlobal, kPolicyNone> */
    OKENV_FORM_GLOBAL_MLP,         /* okStepKernel<kGridGlobal, kPolicyMlp> */
    OKENV_FORM_BRUTE,              /* okStepKernel<kGridBrute, kPolicyNone> */
    OKENV_FORM_BRUTE_MLP,          /* okStepKernel<kGridBrute, kPolicyMlp> */
    OKENV_NUM_STEP_FORMS
};
/* Attributes of a launch, counted beside its form. */
enum okenv_step_form_attr {
    OKENV_FORM_ATTR_FRONT_BACK,       /* walked the front / back images */
    OKENV_FORM_ATTR_LIST,             /* stepped an episode list */
    OKENV_FORM_ATTR_WIDENED,          /* Q-learning list launched with wider lane groups than the handle's */
    OKENV_FORM_ATTR_CTRL_LDS,         /* controller parameters staged in LDS */
    OKENV_FORM_ATTR_AGENTS_PER_BLOCK, /* a fixed number of agents per workgroup (okenv_info.agents_per_block > 0) */
    OKENV_NUM_STEP_FORM_ATTRS
};
/* Step-kernel launches of the handle since it was created (or last cleared), by form: out[f * (1 + OKENV_NUM_STEP_FORM_ATTRS)]
 * counts the launches of form f, the OKENV_NUM_STEP_FORM_ATTRS words after it those of them with each attribute.  n_words must
 * be at least OKENV_NUM_STEP_FORMS * (1 + OKENV_NUM_STEP_FORM_ATTRS); clear != 0 zeroes the counts after copying them. */
OKENV_API int okenv_debug_step_forms(okenv_t h, uint64_t *out, int32_t n_words, int32_t clear);

/* The launch policy of openkitchen_amd/csrc/okenv_capi.hip on plain numbers, no handle and no GPU needed (as okenv_expert_act_host):
 * what okenv_create would decide for a population, and what the launcher would do with one call on it.  For the tests, which run
 * the rules this way for compute-unit counts and image sizes no device at hand shows. */
#define OKENV_PLAN_FIRST_ROLLOUT (-2)
typedef struct okenv_plan_query {
    int32_t  num_agents, num_rays, compute_units;
    uint32_t flags;            /* okenv_create's */
    int32_t  image_fits_lds;   /* what the grid builder says of the track */
    /* the OKENV_* launch variables as numbers; the value that stands for "unset" in brackets */
    int32_t  lanes_per_agent;  /* [0] */
    int32_t  block_threads;    /* [0] */
    int32_t  coop;             /* [1] */
    int32_t  agents_per_block; /* [-1] */
    int32_t  tail_max_agents;  /* [-1] */
    int32_t  resident;         /* [-1] */
    int32_t  front_back;       /* [1] */
    float    phase1_range;     /* [-1] */
    /* bytes of the track image, of the front / back images (0: the track has no split), of the centre line in LDS */
    int32_t  image_bytes, front_back_bytes, q_bytes;
    /* the call */
    int32_t  action_source;    /* 0 stored actions, 1 okenv_rollout_random, 2 MLP policy, 3 Q-learning, 4 controller */
    int32_t  n_listed;         /* agents on the episode's list, -1: no list, OKENV_PLAN_FIRST_ROLLOUT: an episode's first rollout */
    int32_t  packed;           /* okenv_step_packed */
    int32_t  resident_launch;  /* ... starting its resident kernel */
    int32_t  do_move;
    uint32_t reset_flags;
    int32_t  ctrl_num_params;
} okenv_plan_query;
typedef struct okenv_plan_result {
    /* the handle's shape */
    int32_t lanes_per_agent, natural_lanes, rays_per_lane;
    float   phase1_range, grid_cell; /* grid_cell: the default cell edge */
    int32_t grid_mode;               /* 0 LDS image, 1 global grid, 2 brute force */
    int32_t front_back_built, block_threads, grid_blocks, coop, agents_per_block, tail_max_agents, resident_mode, resident_eligible;
    int32_t tail_limit;              /* for this call's policy (okenv_episode_tail_limit) */
    /* the launch */
    int32_t form;                    /* enum okenv_step_form */
    int32_t launch_grid, launch_block, launch_lds_bytes, launch_image_off;
    float   launch_phase1;
    int32_t launch_lanes, launch_front_back, launch_ctrl_lds_off, launch_waves;
} okenv_plan_result;
OKENV_API int okenv_debug_plan_step(const okenv_plan_query *query, okenv_plan_result *out);

#ifdef __cplusplus
}
#endif
#endif /* OKENV_H */
