/* vfik.h -- C-ABI of the MI355X-native batched closed-loop IK path (libvfik_hip.so).
 *
 * The reference (arcoslab/vfclik) has no FFI: its per-cycle path is a set of Python processes
 * (scripts/vf, scripts/nullspace, scripts/debug_jointlimits, src/command_mixer.py inside
 * scripts/bridge) that exchange YARP bottles.  This header is the boundary a maintainer would bind
 * (ctypes) to replace the body of those loops for B arms at once.  Each entry
 * point names the reference code it stands in for (file:line under the reference tree).
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no torch / HIP types in any signature (a HIP stream is
 *     passed as void*).
 *   - every function returns 0 on success or a negative VFIK_E_* code; vfik_last_error() gives
 *     the text for the calling thread.  Bad input is never fatal -- like the reference, which
 *     logs and ignores malformed bottles (scripts/vf:176-179,204-207,264-266).
 *   - per-arm numeric trouble (NaN, limit stop, ...) is reported in status[B] (VFIK_ST_*),
 *     never by failing the call (src/command_mixer.py:71-75 only prints).
 *     Non-finite inputs stay inside their arm.  Three sentences hold for every cycle kernel, the rollout and the five timed moves, and the
 *     suite holds every built kernel variant to them (tests/test_gpu_poison_isolation.py, tests/test_gpu_poison_moves.py):
 *       C1, isolation.  Two runs whose inputs differ only in rows of a set P of arms give the arms outside P the same BITS in every
 *           output row and in every piece of per-arm device state (as the next clean cycle's outputs show it); in a timed move also
 *           arrived / reached, q_traj, dist_traj, diff, the waypoint reports and stalled, and pending[k] differs from the clean run's by
 *           the change in the number of arms of P still under way.
 *       C2, no laundering.  Where the C oracle (oracle/vfik_oracle.c, stepped on the host; a clamp is numpy.clip, which keeps a NaN) has a
 *           NaN or an infinity in an element of a joint-command row (qdot_vf, qdot_null, qdot_out, the q_cmded form) or of the integrated
 *           q (q_out, q_traj) of an arm of P, the library's element is not finite either; where both are finite they agree as for a clean
 *           arm; VFIK_ST_NAN is set exactly where the oracle sets it.  A poisoned arm never arrives, is never reported at a waypoint and
 *           counts in pending as an arm under way (until a stall rule declares it stalled: NaN is never progress).  pose, v6, qdist and
 *           goal_dist of such an arm are specified only where both sides are finite: the kernels skip arithmetic on a chain's structural
 *           zeros, where the oracle's general product has 0 * NaN.
 *       C3, recovery.  No NaN is kept: once the inputs are finite again the arm's rows are the oracle's from the first cycle on, with no
 *           vfik_reset_state -- the nullspace sign memory of a cycle without a usable Jacobian is left as it was --; io->track_error shows an
 *           input of one cycle for three more calls (the command of three calls ago), io->obj_dist for none.
 *     A goal or repeller row of vfik_move_fields whose FIRST element is finite and a later one NaN or infinite: a goal position or a repeller
 *     row that is not finite makes the arm's commands NaN with VFIK_ST_NAN (a NaN is no short distance: the field's sum keeps it); a goal
 *     ROTATION that is not finite is swallowed by the specification -- the angle fails vf's compare, the goal turns the arm nowhere, no NaN
 *     reaches a command and VFIK_ST_NAN stays clear (tests/poison_reference.py: SWALLOWED, with the oracle's lines).
 *   - batch arrays are batch-major: q[B][n], qdot[B][n], pose[B][16], ...  Element type is the
 *     handle's io dtype (float for 32, double for 64).  Arithmetic is always float64.
 *   - one host thread per handle; one handle per device (shards are independent).
 *   - there is no CPU implementation behind this ABI.  Without a GPU vfik_create fails.
 */
#ifndef VFIK_H
#define VFIK_H

#include <stddef.h>
#include <stdint.h>

#include "vfik_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VFIK_ABI_VERSION 6

enum {
    VFIK_OK = 0,
    VFIK_E_ARG = -1,         /* bad argument (size, NULL, range); nothing was changed */
    VFIK_E_HIP = -2,         /* a HIP runtime call failed */
    VFIK_E_UNSUPPORTED = -3, /* e.g. a joint count the library was not built for */
    VFIK_E_STATE = -4        /* call order (chain not set, ...) */
};

typedef struct vfik_handle vfik_handle;

int vfik_abi_version(void);
/* sizeof(vfik_field), sizeof(vfik_chain), sizeof(vfik_params), sizeof(vfik_io) as this library was built:
 * a binding compares them with its own mirrors before the first call */
void vfik_struct_sizes(size_t out[4]);
const char* vfik_last_error(void);
/* number of visible HIP devices (0 without a GPU; never initialises a context) */
int vfik_device_count(void);
/* joint counts this build has kernels for, as a bit mask (bit n set = n joints supported) */
uint32_t vfik_supported_joints(void);

/* One handle = the state that the reference spreads over one vf, one nullspace, one
 * debug_jointlimits and one bridge/CommandMixer process PER ARM, for `batch` arms on one GPU:
 * field sets (vf:145), sticky tool frames (vf:154), IK weights, nullspace sign state
 * (nullspace:91-92), mixer weights and last commands (command_mixer.py:39-44).
 * io_dtype: 32 or 64.  max_slots: capacity of the per-arm field list in device slots
 * (a repeller takes 1, hemisphere/funnel 2, an extra attractor 3; the first attractor is free). */
vfik_handle* vfik_create(int device, int io_dtype, int n_joints, int max_slots, int batch);
void vfik_destroy(vfik_handle* h);

/* Run on the caller's HIP stream (e.g. torch's current stream) instead of the handle's own.
 * The pointer is used as given: NULL selects the device's default (null) stream. */
int vfik_set_stream(vfik_handle* h, void* hip_stream);

/* Lafik(config) (vf:153, nullspace:60, debug_jointlimits:56): chain geometry + joint limits. */
int vfik_set_chain(vfik_handle* h, const vfik_chain* chain);

/* speedScale (/max_vel, vf:197-207), 't'/'j' weights (/weight, vf:295-309), nullspace gain and
 * look-ahead (nullspace:62,121), mixer weights (/bridge/weight, command_mixer.py:48-53), bridge
 * max_vel (bridge:612-623), feature flags.  Range checks of the ports are done by the host layer. */
int vfik_set_params(vfik_handle* h, const vfik_params* p);

/* Per-arm speedScale: what each arm's vf keeps after a /max_vel message (vf:197-207).  values[n_arms]
 * for arms [first_arm, first_arm + n_arms).  vfik_set_params.speed_scale writes one value to all arms. */
int vfik_set_speed_scale(vfik_handle* h, int first_arm, int n_arms, const double* values);

/* /tool (vf:321-326): 16 doubles row-major, shared by the batch (per_arm = 0) or tool16[B][16].  ONE tool for the batch keeps the
 * launches of an all-revolute chain on the kernels built for such chains (the lean and publishing-lean float32-I/O
 * variants apply it themselves); per-arm tools take the general variants.  A per-arm array whose rows are all equal IS a
 * shared tool and is stored as one (with the values rounded to the I/O type, as the per-arm image would hold them).
 *
 * What a tool may be: ANY twelve numbers, as for KDL's frame product (vf:329-332).  Nothing is checked and nothing is assumed of the
 * 3 x 3 block -- a tool read from a float32 file or typed with four decimals is off a rotation by 5e-8 ... 1e-4, and its transpose is
 * NOT its inverse to the accuracy of the results: pose = flange * tool, the twist is shifted by p_flange - p_tip, and pose_no_tool is
 * the flange frame, for every block.  The kernels that apply the shared tool themselves keep no flange value through the field and
 * rebuild both from the tool pose with the block's INVERSE (the host's, in long double).  The rule for a block that cannot be inverted
 * to working accuracy: a shared tool with max |Rtool Rtool^T - I| > VFIK_TOOL_MAX_DEFECT (1/16: no rigid hand), a singular or a
 * non-finite block is not a tool of those kernels -- the handle takes the general variants (vfik_dh_pattern reports 0), which keep
 * the flange frame and need no inverse.  One exception: chains of 10 joints and more recompose pose_no_tool's ROTATION from the tool
 * pose on the general variants too (they have no registers to keep it), so with a block that has no inverse those nine entries are
 * not finite; its position, pose and every qdot are right. */
int vfik_set_tool(vfik_handle* h, const double* tool16, int per_arm);

/* Field sets of arms [first_arm, first_arm + n_arms): the result of the add/remove bookkeeping of
 * vf:209-275 -- fields[n_arms][max_fields] in the reference's parameter layouts, counts[n_arms].
 * Packing (ascending id; lowest-id attractor -> goal block) happens here, on the host, only when a
 * message arrived, exactly when the reference rebuilds totalVF (vf:276-293). */
int vfik_set_fields(vfik_handle* h, int first_arm, int n_arms, const vfik_field* fields,
                    int max_fields, const int32_t* counts);

/* ABI 6.  Goals and obstacles that MOVE.  The reference's object feeder re-sends every primitive of an object whenever the object's pose
 * changes (object_feeder:214-354: the goal attractor, object_feeder:229-241; the point obstacles and the near-goal repeller,
 * object_feeder:317-334): same ids, types, forces, safe distances and orders, new coordinates.  vfik_move_fields rewrites those
 * coordinates inside the device images that vfik_set_fields packed, with one small kernel on the handle's stream: no host pack, no
 * host synchronisation, and no allocation after the first call.  Device pointers, io dtype, asynchronous: the call is ordered after
 * the launches enqueued before it and before those enqueued after it; like the setters it first waits for outstanding
 * vfik_submit_host tickets, and has no other host wait.
 *   goal16 [n_arms][16]  row-major 4x4, the layout of io->pose (a leader's io->pose buffer may be passed as it is), or NULL: goals
 *          stay.  Rows 0-2 replace the frame of the arm's goal block -- its lowest-id attractor.  Slow-down distance, force, the
 *          `present` flag and the arm's speedScale are not touched.  An arm without a goal block ignores its row.
 *   rep4   [n_arms][n_rep][4] = x y z radius, or NULL.  Row k replaces x y z radius of the arm's k-th decay repeller
 *          (VFIK_FIELD_REPELLER) in ASCENDING-ID order; safe distance, force and order stay.  Rows with k at or beyond the arm's
 *          repeller count are ignored (unused slots keep what disarms them).
 *   A goal row or a repeller row whose FIRST element is NaN leaves that primitive as it is (the convention of io->q_ref);
 *   active [n_arms] (device, may be NULL): active[b] == 0 leaves the whole arm as it is.
 * The caller keeps radius >= 0 and radius + safe distance >= 0, as the fields it handed to vfik_set_fields did (the uniform repeller
 * image relies on it).  NOT moved by this call: funnels, hemispheres and attractors beyond the first -- those move with vfik_move_scene.
 * Every image a later launch may read carries the new values (goal block, uniform, compact and general slot images): lean and
 * publishing launches, rollouts, launches with per-arm options, vfik_probe_field and io->goal_dist all see the moved scene.  Nothing a
 * launch decides at enqueue time changes: vfik_field_path, vfik_uniform_repellers, vfik_mixed_orders, vfik_slots_in_use and
 * vfik_launch_epoch keep their values, and a captured graph that contains vfik_step stays valid.
 * VFIK_E_ARG: bad arm range, both arrays NULL, n_rep < 0 or n_rep > max_slots; VFIK_E_STATE: no vfik_set_fields call yet. */
int vfik_move_fields(vfik_handle* h, int first_arm, int n_arms, const void* goal16, const void* rep4, int n_rep, const int32_t* active);
/* The same with HOST arrays of doubles, rounded to the io dtype exactly as vfik_set_fields rounds vfik_field.p[]; copies, launches and
 * synchronises (a setter, like vfik_set_fields -- at a fraction of its cost: nothing is sorted or packed). */
int vfik_move_fields_host(vfik_handle* h, int first_arm, int n_arms, const double* goal16, const double* rep4, int n_rep);

/* The whole scene of a moving object.  `set goalAndNormal` (object_feeder:248-303) re-sends the goal attractor, the approach FUNNEL and the
 * near-goal repeller when the target's pose changes; `set ObstacleH` (object_feeder:335-354) re-sends a HEMISPHERE, a surface with its
 * normal.  vfik_move_scene is vfik_move_fields -- the same ordering on the handle's stream, the same wait for vfik_submit_host tickets and
 * no other, no allocation, the same NaN / active / ragged-row rules, and nothing a launch decides at enqueue time changes -- for all of:
 *   goal16, rep4, n_rep, active   as vfik_move_fields.
 *   fun6   [n_arms][n_fun][6] = x y z ax ay az: apex and axis of the arm's k-th funnel (VFIK_FIELD_FUNNEL) in ascending-id order.  Cut
 *          angle, angle order, cut distance, distance order and force stay.
 *   hem6   [n_arms][n_hem][6] = x y z nx ny nz: plane point and normal of the arm's k-th hemisphere (VFIK_FIELD_HEMISPHERE) in
 *          ascending-id order.  Safe distance, order and force stay.
 *   att16  [n_arms][n_att][16]  row-major 4x4: rows 0-2 replace the frame of the arm's k-th attractor AFTER the goal block (ascending
 *          id).  The frame's last row, the slow-down distance and the force stay.
 * Any array may be NULL: that class stays.  A row whose first element is NaN leaves its primitive as it is; rows at or beyond the arm's
 * count of that class are ignored.  The general slot image carries every row; the straight-line path's aux block carries the arm's first
 * funnel and first hemisphere, so row 0 of fun6 / hem6 is written there too.
 * VFIK_E_ARG: bad arm range, all five arrays NULL, a count < 0 or > max_slots (or, host form, `active` given); VFIK_E_STATE: no
 * vfik_set_fields call yet. */
typedef struct vfik_scene_move {
    const void* goal16;
    const void* rep4;
    const void* fun6;
    const void* hem6;
    const void* att16;
    const int32_t* active;
    int32_t n_rep, n_fun, n_hem, n_att;
} vfik_scene_move;
/* sizeof(vfik_scene_move) as this library was built (vfik_struct_sizes keeps its four entries) */
size_t vfik_scene_move_size(void);
int vfik_move_scene(vfik_handle* h, int first_arm, int n_arms, const vfik_scene_move* mv);
/* The same with HOST arrays of doubles (mv->active must be NULL), rounded to the io dtype exactly as vfik_set_fields rounds
 * vfik_field.p[]; copies, launches and synchronises, like vfik_move_fields_host. */
int vfik_move_scene_host(vfik_handle* h, int first_arm, int n_arms, const vfik_scene_move* mv);

/* Per-arm IK weights: what each arm's vf process keeps after a /weight message (vf:164-179,295-309): 't' + 6
 * task-space weights -> wy[n_arms][6], 'j' + n joint-space weights -> wq[n_arms][n]; either may be NULL
 * (unchanged).  Arms never written use vfik_params.wy / wq; a later vfik_set_params that CHANGES wy or wq
 * is batch-wide again and replaces every arm's own weights.  A call for the WHOLE batch with both arrays whose rows are all equal is a
 * batch-wide setting too (kept by the handle beside the caller's vfik_params, the arms' own weights dropped; a later vfik_set_params
 * whose wy / wq equal what the caller passed last leaves them in force): batch-wide weights keep the launches of an
 * all-revolute chain of up to 7 joints on the kernels built for it, per-arm weights take the general variants. */
int vfik_set_arm_weights(vfik_handle* h, int first_arm, int n_arms, const double* wy, const double* wq);

/* Per-arm mixer weights, w[n_arms][6]: what each arm's bridge keeps after a /bridge/weight message
 * (command_mixer.py:48-53; handlers send [cart, null, joint, 0], handlers.py:189-204).  NULL returns every
 * arm's weights to the batch-wide vfik_params.mix_w (per-arm limiter speeds of vfik_set_max_vel stay).  A
 * vfik_set_params that CHANGES vfik_params.mix_w writes the new weights to every arm.  While every arm's bridge state (these weights and the
 * limiter speed of vfik_set_max_vel) is the same, launches read it from the batch constants as if it had never been set per arm, and keep
 * the kernel variants without per-arm options (every handler sends the same [cart, null, joint, 0] at start-up: handlers.py:189-204,481-497). */
int vfik_set_mixer_weights(vfik_handle* h, int first_arm, int n_arms, const double* w);

/* Per-arm limiter speed: what each arm's bridge keeps after a /bridge/max_vel message (bridge:612-623; the
 * reference accepts 0 <= v <= config.max_vel, the caller applies that rule).  Used with VFIK_F_LIMITER.  Any
 * v >= 0, +inf included (no limit: the decision is lead > max_vel), as for vfik_params.max_vel; negative values
 * and NaN are refused.  A vfik_set_params that CHANGES vfik_params.max_vel writes the new value to every arm. */
int vfik_set_max_vel(vfik_handle* h, int first_arm, int n_arms, const double* values);

/* Last command of mixer channel 2..5 (jointcmd, mechanismcmd, xtra1cmd, xtra2cmd; bridge:593-596)
 * for the whole batch: host array cmd[B][n] in the io dtype, or NULL to zero the channel, which is
 * also what the watchdog does after guard_time of silence (command_mixer.py:64-66). */
int vfik_set_ext_cmd(vfik_handle* h, int channel, const void* cmd_host);

/* Forget the nullspace sign memory (sig = 1, lastvec = 0; nullspace:91-92). */
int vfik_reset_state(vfik_handle* h);

/* Buffers of one control cycle.  NULL = not wanted / not supplied. */
typedef struct vfik_io {
    const void* q;            /* in  [B][n]   /qIn, /nullspace/qin, /debug/qin (vf:312, nullspace:162).  Angles of up to about 1e5 rad: sine and
                                 cosine keep their 1 - 2 ulp.  The kernels built for a chain's DH pattern (lean and publishing-lean launches
                                 of the LWR, two LWRs in series and the 6-joint arm: vfik_dh_pattern) take the angle as it is and publish a
                                 pose within 8 units of the 50-digit kinematics at |q| ~ 10, 1e3 and 1e5 (a unit: 2^-53 per joint).  Every
                                 other kernel -- launches with per-arm options, chains off a pattern, the eight-lanes kernel -- ADDS a link's
                                 DH angle offset to the joint angle in double: each joint with a nonzero offset carries up to
                                 (|q| + |offset|) 2^-53 rad, 1.6e-11 in the pose at 1e5 rad (tests/test_gpu_far_angles.py holds both to their
                                 bars).  Finite angles beyond 1e5 rad are outside the contract.  NaN and +-inf: the
                                 arm's commands are NaN and VFIK_ST_NAN is set (C1 - C3 above). */
    const void* null_control; /* in  [B][4]   /nullspace/control (nullspace:169-173); NULL = zeros.  HONOURED ONLY where the
                                 nullspace is one-dimensional (7 joints at a regular pose: element 0 scales the unique
                                 basis vector, nullspace:110-117).  With nullity >= 2 -- every chain of 8+ joints, a
                                 7-joint arm at a rank-deficient pose -- the reference moves along whatever basis LAPACK's
                                 SVD returns inside the nullspace, which cannot be restated: the arm then gets
                                 VFIK_ST_NULL_AMBIGUOUS, /control contributes nothing, and qdot_null carries the
                                 joint-limit task alone.  What IS reproduced there is the subspace: the reference's
                                 command lies in null(J) and the projector used here leaves it unchanged
                                 (tests/test_oracle_golden.py, the reference's own n = 14 outputs).
                                 THE RANK DECISION next to a singular pose, in terms of sigma_6 / sigma_1 of J:
                                 up to 7 joints, a row of J is kept while its residual is above 1e-12 of its length, the reference's
                                 pinv keeps what is above 1e-15: below sigma_6 / sigma_1 = 1e-10 the decision (hence nullity, status
                                 and qdot_null) is the implementation's own, above it qdot_null is the reference's to within
                                 eps sigma_1 / sigma_6.  8 and more joints: the joint-limit task is projected off the rows of J
                                 that pass VFIK_PROJ_ROW_MIN (vfik_types.h) -- a row within 1e-3 of the span of the rows before it
                                 is dropped, so from about sigma_6 / sigma_1 = 1e-3 down the projected task keeps a component of
                                 up to 1e-3 sigma_1 |z| in task space that the reference's pinv would remove; the C oracle
                                 states the same rule, and the decision is the implementation's own only where a row sits within
                                 a factor of 4 of the threshold (tests/hp_nullspace.py) */
    void* qdot_vf;            /* out [B][n]   /vectorField/qdotOut (vf:462-466) */
    void* qdot_null;          /* out [B][n]   /nullspace/qdotout (nullspace:180-184) */
    void* qdot_out;           /* out [B][n]   mixed (+limited) command (bridge:626); = qdot_vf without the mixer */
    void* pose;               /* out [B][16]  /pose (vf:341) */
    void* pose_nt;            /* out [B][16]  /pose_no_tool (vf:342) */
    void* v6;                 /* out [B][6]   field twist before RefPoint (vf:346-347; /vector_out) */
    void* qdist;              /* out [B][n]   distToCenter (debug_jointlimits:65-67), not x100 */
    int32_t* status;          /* out [B]      VFIK_ST_* */
    void* goal_dist;          /* out [B][2]   xyz distance and rotation angle in DEGREES to the goal: the object-0
                                 entry of /dmonitor/distOut (monitor_distance:76-84,161-172) */
    const void* q_ref;        /* in  [B][n]   /jpctrl/ref (joint_p_controller:113-118); NULL = no joint controller.
                                 An arm whose row starts with NaN has no controller either: its channel 2 stays the
                                 external /bridge/jointcmd command of vfik_set_ext_cmd.
                                 With VFIK_F_MIXER the controller's output kp*(clamp(ref,limits) - q)
                                 (joint_p_controller:89-99,124-128) IS mixer channel 2 (/bridge/jointcmd,
                                 joint_p_controller:78) and an external channel-2 command is not read */
    const void* q_cmded;      /* in  [B][n]   the LWR's echo of its last commanded position (bridge:168-172);
                                 NULL = velocity command.  With it qdot_out is the LWR command form
                                 -q_cmded + q + qdot_lim (bridge:199-203) unless all mixer weights of the arm
                                 are 0 ("direct_control", bridge:604).  vfik_step only */
    /* ---- ABI 3 ---- */
    const int32_t* active;    /* in  [B]      fresh-q gate, NULL = every arm.  The reference advances an arm only when that
                                 arm's own joint angles arrived (vf:312-313, nullspace:162-163, debug_jointlimits:61): an
                                 arm with active[b] == 0 publishes NOTHING this cycle -- no output row of it is written
                                 (status included) and its nullspace sign memory (nullspace:91-92) stays as it was */
    const void* q_lo;         /* in  [B][n]   joint limits of THIS cycle, per arm; NULL (both) = the chain's static limits. */
    const void* q_hi;         /*              The reference re-reads the limits every cycle because some robots' limits
                                 depend on the configuration (nullspace:167 `rob.get_limits()`, joint_p_controller:80
                                 `config.updateJntLimits(cur_pos)`, :121-125).  Used by check_limits (nullspace:120-131), the
                                 joint controller's clamp (joint_p_controller:79-89), distToCenter (debug_jointlimits:66-67),
                                 the joint-limit task and the rollout's clamp.  lo < hi is the caller's business */
    void* q_ref_out;          /* out [B][n]   the joint controller's reference after its clamp: the reference KEEPS the clamped
                                 value (joint_p_controller:121 `ref = check_limits(ref, indata)`), so with limits that move
                                 a host feeds this back as the next cycle's q_ref.  Only with q_ref */
    /* ---- ABI 4: the observers of the cycle, advanced by the SAME call on the cycle's own device results (no host round
     * trip: the reference's vf computes its tracking error inside the loop body, vf:349-428, and monitor_distance reads
     * the pose vf just published, monitor_distance:148-172).  vfik_step / vfik_step_host / vfik_submit_host only ---- */
    void* track_error;        /* out [B][8]   the /track_error bottle (vf:418-427): vel_diff_angle, rot_diff_angle,
                                 ext_vel_mag_corr, ext_rot_mag_corr, cmd_vel_mag_corr, cmd_rot_mag_corr, ext_int_diff,
                                 arm_tracking; zeros until the 6th frame (vf:354).  Requesting it advances the handle's
                                 per-arm history by one frame (gated arms: nothing, as in vfik_track_error) */
    void* obj_dist;           /* out [B][n_objects][2]  xyz distance and rotation angle in DEGREES between the tool pose and
                                 every object frame of vfik_set_objects -- the entries of /dmonitor/distOut
                                 (monitor_distance:156-167).  Needs vfik_set_objects */
} vfik_io;

/* One control cycle for the whole batch -- the loop bodies of vf:311-466, nullspace:162-184,
 * debug_jointlimits:61-73 and command_mixer.py:78-82 (+ bridge:188-195) in ONE kernel launch.
 * Device pointers; asynchronous on the handle's stream.  io->q may have any alignment of its element type: a q that is not
 * 16-byte aligned is first copied (on the handle's stream) into an aligned buffer of the handle -- the kernels read q in whole
 * 16-byte pieces.  That buffer is allocated at the first such call: a host that captures vfik_step / vfik_rollout with such a q
 * makes one call outside the capture first.  The same holds for vfik_rollout. */
int vfik_step(vfik_handle* h, const vfik_io* io);
/* Same with host pointers: copies in, runs, copies out, synchronises. */
int vfik_step_host(vfik_handle* h, const vfik_io* io);
int vfik_sync(vfik_handle* h);

/* Pipelined host path.  The reference's modules exchange Python lists over ports every cycle
 * (vf:312-315,462-466): for a host that keeps q and qdot in its own memory the copies, not the kernel,
 * bound the rate.  vfik_submit_host is vfik_step_host without the wait; outputs are in host memory after
 * vfik_wait(ticket); up to 3 submissions are in flight; kernels run in submission order on the handle's
 * stream.  With PINNED buffers (vfik_host_alloc, or the caller's own hipHostMalloc / hipHostRegister / torch
 * pin_memory) the kernel writes qdot across PCIe itself (zero-copy); q is read the same way when nothing
 * else is in flight, and moved by the copy engine, overlapping the previous kernel, when something is.
 * With pageable buffers copy-in, kernel and copy-out are staged on three streams.  The io buffers must stay
 * untouched until vfik_wait.  Device pointers are accepted as well (then it is vfik_step + an event). */
void* vfik_host_alloc(vfik_handle* h, size_t bytes);
int vfik_host_free(vfik_handle* h, void* p);
int vfik_submit_host(vfik_handle* h, const vfik_io* io, long* ticket);
int vfik_wait(vfik_handle* h, long ticket);

/* Closed-loop rollout: n_cycles control cycles in ONE launch.  After each cycle the
 * commanded velocity (what io->qdot_out reports) is integrated, q <- q + dt * qdot_out -- the role of
 * the kinematic simulator `joint_sim` that `vfclik -s` wires behind the bridge (scripts/vfclik:99-103,
 * scripts/bridge:136-139) -- and optionally clamped to the joint limits.  io->q is the start
 * configuration; the outputs named in io are those of the LAST cycle; q_out[B][n] (may be NULL) receives
 * the joint angles after it.  Field sets, tools, weights and /control stay fixed during the launch,
 * as they do between two messages in the reference; the nullspace sign memory advances every cycle.
 * All-revolute chains of up to 7 joints whose batch-wide tool is the identity and whose batch-wide IK
 * weights are all 1 run all cycles inside one kernel, q carried in double from cycle to cycle.  Every
 * other handle -- a longer chain, a prismatic joint, a shared tool or batch-wide weights other than
 * those, and ANY per-arm tool or per-arm weight array the handle holds, whatever its values (equal
 * per-arm rows that vfik_set_tool / vfik_set_arm_weights stored as batch-wide ones count as batch-wide):
 * no registers left for loop-carried state -- runs n_cycles single-cycle launches that integrate q on
 * the way out.  Those hand q from launch to launch in the io dtype: the same results at float64 I/O,
 * and at float32 I/O the results of a caller that steps the cycles itself and keeps q in float32 (q is
 * rounded to float32 behind every cycle, not only behind the last one).  A block of vfik_goto and its
 * kin is such a rollout of `stride` cycles.
 * Device pointers, asynchronous; vfik_rollout_host takes host pointers and synchronises. */
int vfik_rollout(vfik_handle* h, const vfik_io* io, int n_cycles, double dt, int clamp_to_limits, void* q_out);
int vfik_rollout_host(vfik_handle* h, const vfik_io* io, int n_cycles, double dt, int clamp_to_limits, void* q_out);

/* Batched goto.  Every user-level motion call of the reference is "send a goal, then wait until the arm is there" (handlers.py:346-440:
 * gotoFrame(frame, wait, goal_precision) -> (result, [pos_dist, orient_dist]); gotThere, gotoPosBlocking; set_ref_js(..., wait,
 * goal_precision), handlers.py:544-576): the handler reads the object-0 entry of /dmonitor/distOut -- io->goal_dist -- until
 * pos_dist < goal_precision[0] and orient_dist * pi / 180 < goal_precision[1] (handlers.py:374-381) or the time is up.  vfik_goto is that wait
 * for the batch, on the device: n_cycles / stride BLOCKS of `stride` control cycles each -- a vfik_rollout of `stride` cycles, with the kernels
 * and the integration of vfik_rollout -- and after every block one small kernel that checks each arm's goal_dist row against the precision
 * (both compares strict, in double; NaN never arrives), notes the cycle of the first success in arrived[], counts the arms still under
 * way in pending[k] and sets the gate of the next block.  The whole sequence is enqueued on the handle's stream with no host round trip.
 *   arrived[b]   = (k + 1) * stride - 1 for the first check k the arm passed: the 0-based index of the cycle whose tool pose was measured
 *                  (forward kinematics of the joint angles after that many integrations); -1: not within n_cycles.
 *   hold         1: an arm that arrived takes no further cycle -- its joint angles, its rows of the io outputs and its nullspace sign memory
 *                  stay as its arrival block left them (the handler returns and sends nothing more); 0: it keeps tracking its goal.
 *   io->active   the caller's gate: such arms never run, never arrive, are not counted in pending[], and their q rows carry io->q.
 *   An arm WITHOUT a goal block never arrives: the check reads the goal block's `present` flag (its goal_dist row is measured against the
 *   zero frame of an empty block, which a tool near the origin would pass).
 *   io outputs   passed to every block: every arm's rows are those of its last evaluated cycle; status ORs over the blocks.  io->goal_dist,
 *                when given, receives the distances of the last check (an arm that did not run its block: of its last).  io->q is never written.
 *   q_traj rows  are the q ping-pong of the blocks when given (block k reads row k - 1, block 0 io->q); else two buffers of the handle.
 * Device pointers, io dtype, asynchronous; like the setters the call first waits for outstanding vfik_submit_host tickets and has no other
 * host wait.  It changes no vfik_set_* state, vfik_launch_epoch does not move, and it launches the cycle kernels vfik_rollout launches.  The
 * handle's own buffers (gate, pending, a distance row, the q pair, the staging of a q row that is not 16-byte aligned) are allocated at the
 * first call that needs them: a host that CAPTURES vfik_goto makes one such call outside the capture first (VFIK_E_STATE otherwise).
 * VFIK_E_ARG, nothing enqueued: o or o->arrived NULL, stride < 1, n_cycles outside [1, 1000000] or no multiple of stride, dt not finite, a
 * precision negative or NaN, io->q_cmded / io->track_error / io->obj_dist given (as vfik_rollout); VFIK_E_STATE: no chain set. */
typedef struct vfik_goto_opts {
    int32_t n_cycles;          /* time-out in control cycles, 1..1000000, a multiple of stride */
    int32_t stride;            /* cycles between two arrival checks, >= 1; n_checks = n_cycles / stride */
    double  dt;                /* as vfik_rollout */
    int32_t clamp_to_limits;   /* as vfik_rollout */
    int32_t hold;              /* 1: an arm that arrived takes no further cycle (its q, its output rows and its nullspace memory stay) */
    double  pos_prec, rot_prec;/* metres, RADIANS: goal_precision of handlers.py:346-387 */
    int32_t* arrived;          /* out [B]  cycle index of the arm's first successful check, -1 = not within n_cycles.  Required */
    int32_t* pending;          /* out [n_checks]  arms still under way after check k; may be NULL (the handle keeps its own) */
    void*   q_out;             /* out [B][n]  joint angles after the last block (held arms: at arrival); may be NULL */
    void*   q_traj;            /* out [n_checks][B][n]  every arm's joint angles after block k; may be NULL */
    void*   dist_traj;         /* out [n_checks][B][2]  goal_dist at check k; may be NULL */
} vfik_goto_opts;
/* sizeof(vfik_goto_opts) as this library was built (vfik_struct_sizes keeps its four entries) */
size_t vfik_goto_opts_size(void);
int vfik_goto(vfik_handle* h, const vfik_io* io, const vfik_goto_opts* o);
/* The same with HOST pointers (io and o alike); copies in, enqueues, copies out, synchronises.  After every poll_checks checks (>= 1;
 * 0 = never) it reads pending[k] back and stops enqueuing once that is 0: a 20 s time-out then costs the time the slowest arm needs.
 * *checks_run (may be NULL) = the number of checks executed; rows of pending, q_traj and dist_traj beyond it are not written. */
int vfik_goto_host(vfik_handle* h, const vfik_io* io, const vfik_goto_opts* o, int poll_checks, int* checks_run);

/* Waypoint lists.  A user of the reference never makes just one gotoFrame call: a pick-and-place script is a list of them -- approach pose, grasp
 * pose, lift pose, place pose -- and the next frame goes out the moment the previous call returned true (handlers.py:346-387).  vfik_follow is
 * vfik_goto for arms that each carry their own list of goal frames, way16[B][W][16]: the same blocks of `stride` cycles, the same gate, and after
 * every block one small kernel (check_kernel<T, JOINT, LIST>, here <T, 0, 1>) that applies vfik_goto's arrival rule -- the same distance row, both compares strict and in
 * double, NaN never arrives, an arm without a goal block never arrives -- and, for an arm it finds at its waypoint w, writes waypoint w + 1 into
 * the arm's goal block in the same kernel.  No host takes part; the whole run is one enqueued sequence.
 *   path length  L_b = the number of leading rows of way16[b] whose FIRST element is not NaN: a NaN row ends the path, so arms may have paths
 *                shorter than W.  An arm with L_b == 0 is kept out exactly like an arm with io->active[b] == 0: it does not run, is not counted
 *                in pending[], and its goal block is not touched.
 *   before block 0   reached = -1, next = 0, and rows 0..2 of waypoint 0 go into the goal block's frame of every arm that takes part and HAS a
 *                goal block -- the stores of vfik_move_fields; slow-down distance, force, the `present` flag and the arm's speedScale stay.  An
 *                arm without a goal block runs, never arrives and is never written to, as in vfik_goto and vfik_move_fields.
 *   after block k    the precision pair is (via_pos_prec, via_rot_prec) while next[b] < L_b - 1 and (pos_prec, rot_prec) at the arm's last
 *                waypoint.  On success reached[b][next] = (k + 1) * stride - 1 and next += 1; if next < L_b, the frame of waypoint `next` goes into
 *                the goal block.  An arm advances by at most ONE waypoint per check: the distance to the new goal exists only after the next
 *                block (gotoFrame discards its first read for the same reason, handlers.py:365-384).
 *   gate         of the next block: the caller's && L_b > 0 && !(hold && next == L_b).  pending[k] counts the arms that take part and have
 *                next < L_b.  Rows of an arm that did not run its block repeat, as in vfik_goto: q_traj, dist_traj and way_traj.
 *   afterwards   the goal block of an arm holds waypoint min(next, L_b - 1).  Like vfik_move_fields the call changes the goal image only: no
 *                other vfik_set_* state changes, vfik_launch_epoch does not move, no launch decision changes, and it launches only the cycle
 *                kernels vfik_rollout launches.
 * Only a goal that is the plain goal block is supported: a funnel or a near-goal repeller of a goalAndNormal scene (object_feeder:248-303) stays
 * where vfik_set_fields or vfik_move_scene put it.
 * Device pointers, io dtype, asynchronous; io outputs, q_out, q_traj, dist_traj, the wait for vfik_submit_host tickets and the allocation of the
 * handle's buffers (vfik_goto's and one path length per arm: before the first enqueue, never under capture -- VFIK_E_STATE) as vfik_goto.
 * VFIK_E_ARG, nothing enqueued: what vfik_goto refuses, and n_way < 1, way16 / reached / next NULL, way16 not 16-byte aligned, a via_*
 * precision negative or NaN. */
typedef struct vfik_follow_opts {
    int32_t n_cycles, stride;         /* as vfik_goto_opts */
    double  dt;
    int32_t clamp_to_limits, hold;    /* hold: an arm that reached its LAST waypoint takes no further cycle */
    double  pos_prec, rot_prec;       /* metres, radians: the rule at an arm's last waypoint */
    double  via_pos_prec, via_rot_prec; /* the rule at every waypoint before an arm's last one */
    int32_t n_way;                    /* W >= 1 */
    const void* way16;                /* in  [B][W][16], io dtype, 16-byte aligned: the goal frames in order */
    int32_t* reached;                 /* out [B][W]  cycle index of the check that found the arm at waypoint w, -1.  Required */
    int32_t* next;                    /* out [B]     number of waypoints reached = index of the one under way.  Required */
    int32_t* pending;                 /* out [n_checks] arms that have not reached their last waypoint; may be NULL */
    void*   q_out; void* q_traj; void* dist_traj;   /* as vfik_goto_opts */
    int32_t* way_traj;                /* out [n_checks][B] the waypoint index row k of dist_traj was measured against; may be NULL */
} vfik_follow_opts;
/* sizeof(vfik_follow_opts) as this library was built (vfik_struct_sizes keeps its four entries) */
size_t vfik_follow_opts_size(void);
int vfik_follow(vfik_handle* h, const vfik_io* io, const vfik_follow_opts* o);
/* The same with HOST pointers (io and o alike), poll_checks and *checks_run as vfik_goto_host: rows of pending, q_traj, dist_traj and way_traj
 * beyond *checks_run are not written. */
int vfik_follow_host(vfik_handle* h, const vfik_io* io, const vfik_follow_opts* o, int poll_checks, int* checks_run);

/* Joint-space goto.  The reference's second motion call, HandleJController.set_ref_js(js, wait, goal_precision) (handlers.py:544-576): it sends a
 * joint reference to /jpctrl/ref -- io->q_ref -- and reads /bridge/encoders until
 *     ((js - goal_precision) <= q) * ((js + goal_precision) >= q)).all()
 * or the time is up, and returns (result, js - q).  vfik_goto_js is that wait for the batch: the blocks of vfik_goto unchanged -- `stride` cycles
 * through the kernels of vfik_rollout, under the handle's gate, the same q ping-pong or q_traj rows -- and after every block one small kernel
 * (check_kernel<T, 1, 0>) that applies the reference's rule to each arm that ran the block and has not arrived, in double on the io-typed values:
 *     ok = for all i:  (ref[i] - prec[i]) <= q[i]  &&  (ref[i] + prec[i]) >= q[i]
 * Both compares are non-strict and the two edges are computed as written (|ref - q| <= prec is another function in floating point).  q is the
 * block's integrated row -- what /bridge/encoders would publish; ref is the arm's row of io->q_ref AS THE CALLER SENT IT, not the clamped value the
 * controller keeps (io->q_ref_out): a reference beyond a limit by more than its precision never arrives, as in the reference.  NaN in q or in
 * the row never arrives; an arm whose row STARTS with NaN has no controller (the io->q_ref convention): it runs, never arrives and counts in
 * pending[], like an arm without a goal block in vfik_goto.  There is no check in front of block 0.
 *   arrived[b]   = (k + 1) * stride - 1 for the first check k the arm passed, the number vfik_goto gives for check k: the 0-based index of the
 *                  last cycle taken before the joint angles that passed; -1: not within n_cycles.
 *   diff[b][i]   = (T)(ref[i] - q[i]), written at every check the arm ran: set_ref_js's `difference`.  Held and gated arms keep their row.
 *   hold, io->active, pending[k], the io outputs (status ORs over the blocks, io->q is never written), q_out, q_traj, the wait for
 *   vfik_submit_host tickets and the allocation of the handle's buffers (never under capture: VFIK_E_STATE): as vfik_goto.
 * The cycle kernel is the one a vfik_rollout with this io launches, the same for every block; it is asked for goal_dist only when io names it
 * (the rule does not read it).  The mixer flag, the mixer weights (vfik_set_params, vfik_set_mixer_weights: what set_joint_control sends,
 * handlers.py:189-211) and the fields are the caller's: WITHOUT VFIK_F_MIXER the reference moves nothing, as in vfik_step, and the check is
 * made all the same.  vfik_launch_epoch does not move.
 * VFIK_E_ARG, nothing enqueued: what vfik_goto refuses, io->q_ref NULL, prec NULL or an element of it negative or NaN. */
typedef struct vfik_goto_js_opts {
    int32_t n_cycles, stride;      /* as vfik_goto_opts */
    double  dt;
    int32_t clamp_to_limits, hold;
    const double* prec;            /* HOST [n]: goal_precision of handlers.py:544-576, radians (metres for a prismatic joint); each >= 0, not NaN,
                                      +inf allowed (that joint never decides).  Read during the call, in the device form too */
    int32_t* arrived;              /* out [B], required */
    int32_t* pending;              /* out [n_checks], may be NULL */
    void*   q_out;                 /* out [B][n] */
    void*   q_traj;                /* out [n_checks][B][n] */
    void*   diff;                  /* out [B][n]  js - q of the arm's last check: set_ref_js's `difference`; may be NULL */
} vfik_goto_js_opts;
/* sizeof(vfik_goto_js_opts) as this library was built (vfik_struct_sizes keeps its four entries) */
size_t vfik_goto_js_opts_size(void);
int vfik_goto_js(vfik_handle* h, const vfik_io* io, const vfik_goto_js_opts* o);
/* The same with HOST pointers (io and o alike); poll_checks and *checks_run as vfik_goto_host. */
int vfik_goto_js_host(vfik_handle* h, const vfik_io* io, const vfik_goto_js_opts* o, int poll_checks, int* checks_run);

/* Posture lists: vfik_follow's state machine with vfik_goto_js's rule, for arms that each carry a list of joint references wayq[B][W][n] -- the
 * home posture, the pre-grasp posture, ... of a script of set_ref_js calls.  len, reached, next, way_traj, one advance per check, the via / last
 * precision and the gate (the caller's && L_b > 0 && !(hold && next == L_b)) are vfik_follow's; a row of wayq whose FIRST element is NaN ends the
 * arm's list.  The reference row every block reads as io->q_ref belongs to the HANDLE ([B][n], io dtype, allocated with the other goto buffers):
 * in front of block 0 posture 0 goes into it -- an arm that does not take part gets a row that starts with NaN --, and the check that finds an arm
 * at posture `next` writes the following one (check_kernel<T, 1, 1>).  Nothing else of the handle changes: the goal image, vfik_launch_epoch and the
 * launch decisions stay, the cycle kernel is the one a caller's own q_ref would select, and a later call with the caller's own io->q_ref never
 * sees the handle's row.  diff is measured against the posture the arm was sent to, min(next, L_b - 1) on entry to the check.
 * VFIK_E_ARG, nothing enqueued: what vfik_goto refuses, io->q_ref GIVEN (the handle supplies it), n_way < 1, wayq / reached / next NULL, wayq
 * not aligned to its element type, prec NULL, an element of prec or via_prec negative or NaN. */
typedef struct vfik_follow_js_opts {
    int32_t n_cycles, stride;      /* as vfik_goto_opts */
    double  dt;
    int32_t clamp_to_limits, hold; /* hold: an arm that reached its LAST posture takes no further cycle */
    const double* prec;            /* HOST [n]: the rule at an arm's last posture */
    const double* via_prec;        /* HOST [n]: at those before it; NULL = prec */
    int32_t n_way;                 /* W >= 1 */
    const void* wayq;              /* in  [B][W][n], io dtype, element-aligned: a row whose FIRST element is NaN ends the arm's list */
    int32_t* reached;              /* out [B][W], required */
    int32_t* next;                 /* out [B], required */
    int32_t* pending;              /* out [n_checks], may be NULL */
    void*   q_out;                 /* out [B][n] */
    void*   q_traj;                /* out [n_checks][B][n] */
    void*   diff;                  /* out [B][n], may be NULL */
    int32_t* way_traj;             /* out [n_checks][B] the posture index the arm's check k was made against; may be NULL */
} vfik_follow_js_opts;
/* sizeof(vfik_follow_js_opts) as this library was built (vfik_struct_sizes keeps its four entries) */
size_t vfik_follow_js_opts_size(void);
int vfik_follow_js(vfik_handle* h, const vfik_io* io, const vfik_follow_js_opts* o);
int vfik_follow_js_host(vfik_handle* h, const vfik_io* io, const vfik_follow_js_opts* o, int poll_checks, int* checks_run);

/* Motion scripts: frames and postures in ONE list per arm.  A pick-and-place script of the reference starts and ends with set_ref_js (home
 * posture, pre-grasp posture), sends a list of gotoFrame calls between them, and around each change of kind switches the bridge's
 * controller: HandleBridge.joint_controller() sends [0, 0, 1, 0] to /bridge/weight, cartesian_controller() [1, 1, 0, 0] (handlers.py:189-211,
 * 481-497).  vfik_script is vfik_follow's state machine, step for step, over a list whose items are of either kind:
 *   kind[b][w]   (vfik_types.h) VFIK_STEP_FRAME: way16[b][w] is a goal frame, vfik_follow's rule (both compares strict) with (pos_prec, rot_prec) or the
 *                via pair; VFIK_STEP_POSTURE: wayq[b][w] is a posture, vfik_follow_js's rule as written (both edges non-strict, in double on
 *                the io-typed values, against the posture as the caller sent it) with prec[n] or via_prec[n].  Any other value ends the arm's
 *                script: L_b = the number of leading steps of kind 1 or 2, a zeroed array is "no script", and an arm with L_b == 0 is kept
 *                out like one gated off.  way16 is read only at frame steps, wayq only at posture steps; no NaN convention applies.
 *   send         a frame goes into the arm's goal block (vfik_follow's three quad stores, only where the block's `present` flag is set -- an
 *                arm without a goal block never passes a frame step); a posture goes into the arm's row of the handle's reference row,
 *                which every block reads as io->q_ref; and the mixer weights of channels 0..3 of the step's kind -- mix_frame or mix_posture
 *                -- go into the arm's row of two quad planes of the handle's own, which every block reads as the per-arm mixer weights.
 *                Until an arm's first posture its reference row starts with NaN: no controller, channel 2 stays the external command
 *                (io->q_ref).  Over the frame steps behind a posture the row keeps that posture.
 *   before block 0   reached = -1, next = 0, the gate, step 0 sent for every arm that takes part; weights 4, 5 and max_vel of every arm
 *                from its vfik_set_mixer_weights / vfik_set_max_vel row where the handle has one, else the batch-wide vfik_params values.
 *   after block k    the rule of the kind of step next[b] on every arm that ran; on success reached[b][next] = (k + 1) * stride - 1,
 *                next += 1 and the following step is sent.  At most ONE step per check.  The via pairs hold at every step but the arm's last.
 *   hold, io->active, pending[k] (arms that take part and have next < L_b), the gate of the next block, q_out, q_traj, way_traj: vfik_follow's.
 *   dist_traj    the block's goal_dist row of every arm that ran, measured against the goal block as it stands: at a posture step the last
 *                frame sent.  diff[b] = (T)(posture - q), written only by checks made at posture steps: at a frame step the arm keeps its row.
 *   afterwards   nothing of the caller's mixer state has moved: the vfik_set_mixer_weights / vfik_set_max_vel rows, vfik_params and
 *                vfik_launch_epoch stay, and a later call reads them as before.  The goal block is left at the last frame sent.  The cycle
 *                kernels are those a vfik_rollout with io->q_ref on a handle with per-arm mixer weights launches.
 * The handle's planes are allocated at the first call with its other goto buffers: never under capture (VFIK_E_STATE).
 * VFIK_E_ARG, nothing enqueued: what vfik_follow refuses, kind / way16 / wayq / reached / next NULL, way16 not 16-byte aligned, wayq not
 * aligned to its element type, a mixer weight that is not finite, a precision negative or NaN, prec NULL, io->q_ref GIVEN (the handle
 * supplies it).  VFIK_E_STATE: the handle's params lack VFIK_F_MIXER -- a script switches controllers through the mixer. */
typedef struct vfik_script_opts {
    int32_t n_cycles, stride;         /* as vfik_goto_opts */
    double  dt;
    int32_t clamp_to_limits, hold;    /* hold: an arm that reached its LAST step takes no further cycle */
    double  pos_prec, rot_prec;       /* frame steps: metres, radians, at an arm's last step */
    double  via_pos_prec, via_rot_prec; /* ... and at every step before it */
    const double* prec;               /* HOST [n]: posture steps, at an arm's last step */
    const double* via_prec;           /* HOST [n]: ... and at every step before it; NULL = prec */
    double  mix_frame[4];             /* mixer weights of channels 0..3 under way to a frame: the reference sends [1, 1, 0, 0] */
    double  mix_posture[4];           /* ... and under way to a posture: [0, 0, 1, 0] */
    int32_t n_way;                    /* W >= 1 */
    const int32_t* kind;              /* in  [B][W] VFIK_STEP_FRAME, VFIK_STEP_POSTURE; any other value ends the arm's script */
    const void* way16;                /* in  [B][W][16], io dtype, 16-byte aligned: read only at frame steps */
    const void* wayq;                 /* in  [B][W][n], io dtype, element-aligned: read only at posture steps */
    int32_t* reached;                 /* out [B][W], required */
    int32_t* next;                    /* out [B], required */
    int32_t* pending;                 /* out [n_checks], may be NULL */
    void*   q_out; void* q_traj; void* dist_traj;   /* as vfik_follow_opts */
    void*   diff;                     /* out [B][n], may be NULL */
    int32_t* way_traj;                /* out [n_checks][B] the step the arm's check k was made against; may be NULL */
} vfik_script_opts;
/* sizeof(vfik_script_opts) as this library was built (vfik_struct_sizes keeps its four entries) */
size_t vfik_script_opts_size(void);
int vfik_script(vfik_handle* h, const vfik_io* io, const vfik_script_opts* o);
/* The same with HOST pointers (io and o alike), poll_checks and *checks_run as vfik_follow_host. */
int vfik_script_host(vfik_handle* h, const vfik_io* io, const vfik_script_opts* o, int poll_checks, int* checks_run);

/* Stalled arms.  The reference has two outcomes for a timed move: the arm arrived, or it is still under way when the time is up (gotoFrame,
 * set_ref_js: handlers.py:346-387, 544-576).  For a batch that keeps ONE arm that will never arrive -- a goal out of reach, a posture beyond a
 * limit, no goal block -- in pending[k] until the time-out, and the early exit of the host forms never fires.  The stall rule is a third outcome,
 * decided on the device inside the checks of all five timed moves.  It is state of the HANDLE, off by default; with the rule off nothing changes:
 * the same check kernels, the same results.
 *   measure      in double on the io-typed values, like the arrival rules.  Cartesian rule (vfik_goto, vfik_follow, a script's frame steps):
 *                d = the distance, a = the angle in radians exactly as the arrival rule forms it, (double)deg * M_PI / 180.0; both NaN for
 *                an arm without a goal block.  Joint rule (vfik_goto_js, vfik_follow_js, a script's posture steps): e = max_i |(double)ref_i -
 *                (double)q_i| over the joints whose precision in force (prec or via_prec) is finite, 0 without such a joint, NaN if any
 *                of them is NaN; ref is the value the caller sent, as in the arrival rule.
 *   state        per arm best[2] (double) and count (int32), the handle's.  The pass in front of block 0 sets best = +inf, count = 0 and
 *                stalled[b] = -1 for EVERY arm; the check that advances an arm to its next list item or script step resets best and count.
 *   after block k    for every arm that ran the block, is under way and did not arrive at this check: progress means
 *                d < best_d - eps_pos || a < best_a - eps_rot     (joint rule: e < best_e - eps_js),
 *                all compares strict, so NaN is never progress.  On progress best becomes the componentwise minimum and count = 0; else
 *                count += 1, and when count == patience the arm is stalled: stalled[b] = (k + 1) * stride - 1.  Arrival goes first: an arm that
 *                arrives at the check where count would reach patience arrives.  An arm without a goal block, or with a NaN reference
 *                row, stalls at check patience - 1.
 *   a stalled arm  has left the state machine: no rule of any kind is applied to it again, arrived, reached and next keep their values, it
 *                is not counted in pending[k], and with stop = 1 the gate of the next block is 0 for it -- its q, its output rows and its
 *                nullspace memory stay and its trace rows repeat, exactly as for an arm held at arrival.  With stop = 0 it keeps taking
 *                cycles unchecked (diff and way_traj are still written for it).  The gate: in && !(hold && next == L) && !(stop && stalled).
 *   stalled      NULL: an array of the handle, read with vfik_stalled_host; else a DEVICE pointer to int32 [B] that every later timed move
 *                writes.  Either way it holds the outcome of the LAST timed move.
 * vfik_set_stall_rule(h, NULL) switches the rule off.  The call allocates the handle's state (never under capture: VFIK_E_STATE), synchronises
 * the handle's stream, moves no launch decision and leaves vfik_launch_epoch alone; a timed move's blocks run the cycle kernels they ran
 * without a rule (with stop = 1 always under the handle's gate, as with hold).  VFIK_E_ARG: patience < 1, stop other than 0 / 1, an eps negative, NaN or infinite,
 * a `stalled` that is no int32-aligned device pointer; the rule in force stays.
 * vfik_stalled_host copies stalled[B] of the last timed move to the host and synchronises; VFIK_E_STATE without a rule, and while the
 * handle's stream is being captured (nothing is enqueued, the capture goes on). */
typedef struct vfik_stall_rule {
    int32_t patience;         /* >= 1: consecutive checks without progress */
    int32_t stop;             /* 1: a stalled arm takes no further cycle */
    double  eps_pos, eps_rot; /* metres, radians; finite, >= 0 */
    double  eps_js;           /* radians (metres: prismatic); finite, >= 0 */
    int32_t* stalled;         /* out [B] DEVICE pointer, or NULL: the handle's own array */
} vfik_stall_rule;
size_t vfik_stall_rule_size(void);
int vfik_set_stall_rule(vfik_handle* h, const vfik_stall_rule* r);   /* NULL: off (the default) */
int vfik_stalled_host(vfik_handle* h, int32_t* out /* host [B] */);  /* synchronises; the last timed move's */

/* Arms as each other's obstacles.  The reference runs one process set per arm -- `left` and `right` instances of the same robot
 * (old/system_start.sh.old:60,237) -- and an arm learns where its neighbour is only as `set ObstacleP` objects that somebody re-sends
 * whenever they move (object_feeder:317-334).  Here a handle carries up to VFIK_MAX_LINK_SPHERES spheres fixed to links of its chain
 * (vfik_link_sphere, vfik_types.h), and vfik_link_points places them from a batch of joint angles ON THE DEVICE, in the exact shape
 * vfik_move_fields takes as rep4 (and vfik_scene_move as its rep4 member): [vfik_link_points; vfik_move_fields; vfik_step] on one stream is
 * the per-cycle form, with no host wait.
 *
 * vfik_set_link_spheres is a setter like vfik_set_fields: it may allocate, synchronises, and moves vfik_launch_epoch.  Frames are those of
 * the PUBLIC chain (vfik_chain's z-normal form), link 0 = the base frame B[0], link n = the flange; a tool is not applied -- add its offset
 * to c on link n.  L = 0 or s == NULL: no spheres.  A new list switches a coupling off (vfik_set_coupling: its buffer has the old list's
 * rows); vfik_set_chain drops the spheres and the coupling.
 * VFIK_E_ARG: L outside 0..16, a link outside 0..n, a centre that is not finite, a radius that is negative or not finite, reserved != 0;
 * VFIK_E_STATE: no chain yet. */
size_t vfik_link_sphere_size(void);
int vfik_set_link_spheres(vfik_handle* h, const vfik_link_sphere* s, int L);

/* For every arm b of the batch: s = src_arm[b] is the arm whose links become b's obstacles (src_arm == NULL: s = b).  q[s][0..n) is widened
 * to double and the chain is walked once in float64; for sphere j in the CALLER's order P = X_link(q_s) c_j, and with xform12 -- [B][12],
 * row-major 3x4 [R_b | t_b]: where the source's base stands as seen from arm b's base, taken as given, rotation or not -- P becomes
 * R_b P + t_b.  Row first_rep + j of rep4[b][n_rep][4] becomes (P, radius_j) rounded to the I/O type.  Rows outside first_rep ..
 * first_rep + L - 1 are NOT written: a caller fills them with NaN once, and vfik_move_fields then leaves those repellers alone.
 *   s < 0 or s >= B   all L rows of the arm are NaN ("leave as it is") and q is not read for it; no index of src_arm is used unchecked.
 *   NaN in q[s]       all L rows of the arm are NaN.
 * Device pointers, io dtype (src_arm int32), asynchronous on the handle's stream, no allocation; ordered like vfik_move_fields: after the
 * launches enqueued before it and before those enqueued after it, and like it the call first waits for outstanding vfik_submit_host
 * tickets.  Nothing a launch decides at enqueue time changes and vfik_launch_epoch does not move.
 * Robots whose arms differ (left and right arms with other chains or bases) take two handles: handle A's vfik_link_points output is handle
 * B's rep4 argument when both run on one stream (vfik_set_stream) or the caller orders them; there is no cross-handle plumbing.
 * VFIK_E_ARG: q or rep4 NULL, rep4 not 16-byte aligned, first_rep < 0, first_rep + L > n_rep, n_rep > max_slots; VFIK_E_STATE: no spheres. */
int vfik_link_points(vfik_handle* h, const void* q, const int32_t* src_arm, const void* xform12, void* rep4, int n_rep, int first_rep);
/* The same with HOST arrays: q [B][n], xform12 [B][12] doubles, rounded to the io dtype as vfik_move_fields_host rounds its rows, src_arm
 * int32 [B]; rep4 [B][n_rep][4] doubles receives rows first_rep .. first_rep + L - 1 (the io-typed values, widened), its other rows are
 * not touched.  Copies, launches and synchronises; the alignment rule does not apply. */
int vfik_link_points_host(vfik_handle* h, const double* q, const int32_t* src_arm, const double* xform12, double* rep4, int n_rep, int first_rep);

/* Coupling inside the timed moves: state of the HANDLE like the stall rule, off by default; with the coupling off nothing changes -- the
 * same launches, the same results.  While one is set, every block k of vfik_goto, vfik_follow, vfik_goto_js, vfik_follow_js and vfik_script
 * enqueues, in front of its cycles, vfik_link_points on the block's INPUT row of joint angles (block 0: io->q, block k: what block k - 1
 * left) into a buffer of the handle, [B][first_rep + L][4], and the launch vfik_move_fields makes for that buffer as rep4: the arm's
 * first_rep-th .. (first_rep + L - 1)-th decay repellers in ascending-id order follow the source arm's links from check to check, with no
 * host taking part; its repellers before first_rep stay (the buffer's rows there are NaN).  An arm that is gated off, held at arrival,
 * stalled or kept out carries its row of joint angles forward, so it is an obstacle at the posture it holds.  After the move the
 * repellers stay where the last block put them.
 *   link_traj   when given, row k receives the L rows per arm block k started from: vfik_link_points of block k's input row with n_rep = L,
 *               first_rep = 0.  The caller sizes it for the n_checks of the moves it runs.
 * vfik_set_coupling allocates the handle's buffer and fills it with NaN (never under capture: VFIK_E_STATE), synchronises and leaves
 * vfik_launch_epoch alone; the moves allocate nothing for it, and a captured stream stays valid.  The pointers are kept, not copied: the
 * arrays stay the caller's and alive while the coupling is set.  vfik_set_coupling(h, NULL) switches it off.
 * VFIK_E_ARG: first_rep < 0, first_rep + L > max_slots, reserved != 0, src_arm / xform12 / link_traj no device pointer of its alignment
 * (int32; the io type; 16 bytes); VFIK_E_STATE: no spheres set.  A timed move under a coupling before any vfik_set_fields: VFIK_E_STATE. */
typedef struct vfik_coupling {
    const int32_t* src_arm;  /* device [B], may be NULL (every arm its own source) */
    const void*    xform12;  /* device [B][12] io dtype, may be NULL */
    int32_t first_rep;       /* the arm's first_rep-th .. (first_rep + L - 1)-th decay repeller, ascending id */
    int32_t reserved;        /* 0 */
    void*   link_traj;       /* device [n_checks][B][L][4] io dtype or NULL: the rows each block started from */
} vfik_coupling;
size_t vfik_coupling_size(void);
int vfik_set_coupling(vfik_handle* h, const vfik_coupling* c);   /* NULL: off (the default) */

/* Link-sphere clearance.  The field is evaluated at one point, the tool: repellers push the hand away from a neighbour's links and do
 * nothing for the elbow.  vfik_link_clearance is the measurement: for every arm b, how much room is left between its OWN link spheres
 * (vfik_set_link_spheres) at q[b] and a set of other spheres, and which pair is the closest.  The reference has no such thing (its arms
 * meet only as re-sent ObstacleP objects).
 *   q      [B][n], pts4 [B][n_rep][4]: DEVICE arrays of the io dtype.  pts4 holds x y z radius rows, the shape vfik_link_points writes and
 *          vfik_move_fields reads: a neighbour's links (this handle's or another handle's on the same stream), the handle's own links
 *          for self-collision, or static obstacles.  Only rows first .. first + count - 1 of an arm are looked at.
 *   walk   the chain is walked once from q[b] in float64, in the frames vfik_link_points uses (the public chain, link 0 the base, link n
 *          the flange, no tool).  Own sphere i, in the CALLER's order, sits at P_i = X_link_i(q_b) c_i; row j (counted from `first`) is
 *          (Q_j, R_j) widened exactly;  d_ij = sqrt(|P_i - Q_j|^2) - r_i - R_j  from the coordinate differences, in float64.
 *   clear  [B] io dtype: the minimum of d_ij over the pairs considered, rounded to the io dtype;  pair [B] int32 or NULL: i * 32 + j of it.
 *   pairs  considered when mask == NULL or bit j of mask[i] is set (a HOST array of L words, read during the call), and row j holds no
 *          NaN: the library's "leave as it is" row is no obstacle.  Ties take the smallest code.  No pair considered: clear = +inf,
 *          pair = -1.  A NaN anywhere in q[b]: clear = NaN, pair = -1.
 * Asynchronous on the handle's stream, no allocation, ordered like vfik_link_points (the wait for outstanding vfik_submit_host tickets
 * included); no launch decision and no epoch moves; valid under stream capture.
 * VFIK_E_ARG: count outside 1..32, first < 0, first + count > n_rep, q / pts4 / clear NULL, pts4 not 16-byte aligned, a mask bit at or
 * beyond count; VFIK_E_STATE: no spheres set. */
int vfik_link_clearance(vfik_handle* h, const void* q, const void* pts4, int n_rep, int first, int count,
                        const uint32_t* mask /* host [L] or NULL */, void* clear /* [B] io dtype */, int32_t* pair /* [B] or NULL */);
/* The same with HOST arrays: q [B][n] and pts4 [B][n_rep][4] doubles, rounded to the io dtype as vfik_link_points_host rounds its rows;
 * clear [B] doubles receives the io-typed values, widened; pair int32 [B] or NULL.  Copies, launches and synchronises; the alignment rule
 * does not apply. */
int vfik_link_clearance_host(vfik_handle* h, const double* q, const double* pts4, int n_rep, int first, int count, const uint32_t* mask,
                             double* clear, int32_t* pair);

/* Arms that wait for room: stop-and-wait by priority inside the timed moves.  State of the HANDLE like the stall rule and the coupling, off
 * by default; with the rule off nothing changes -- the same launches, the same results.  The rule needs a coupling (vfik_set_coupling) and
 * goes when the coupling goes: a new sphere list, vfik_set_coupling(h, NULL), vfik_set_chain.
 * While it is set, every block k of the five timed moves enqueues, after the coupling's two launches and in front of its cycles, the
 * measurement of vfik_link_clearance on the block's INPUT row of joint angles against rows first_rep .. first_rep + L - 1 of the handle's
 * coupling buffer: the partner's links as just placed, NaN for an arm without a source.  It
 *   writes clear_traj[k][b] and pair_traj[k][b] for every arm (where given), and
 *   for an arm with gate[b] == 1 and yields[b] != 0 whose io-typed clearance, widened to double, is < min_clearance: sets gate[b] = 0 for
 *   this block and counts it in waited[b].  The compare is strict: NaN and +inf never wait.  Block 0 stores the count, later blocks add.
 * The check after the block treats a gated arm as one that did not run -- its rows repeat, no arrival rule and no stall rule is applied
 * to it, it stays in pending -- and rewrites the gate from the state machine alone, so a waiting arm runs again as soon as the room is
 * back.  A move under a rule always runs under the handle's gate (as with hold); the *_host forms copy the caller's rows of the gated
 * outputs in first (an arm that waits through block 0 has no distance row of its own yet).
 *   min_clearance  finite.
 *   yields         DEVICE int32 [B] or NULL (every arm): only an arm with yields[b] != 0 ever waits -- the caller's priority tool.
 *   mask           own sphere i against partner sphere j, as in vfik_link_clearance; all sixteen words zero = every pair.
 *   clear_traj, pair_traj   DEVICE [n_checks][B] (io dtype, int32) or NULL; the caller sizes them for the moves it runs.
 *   waited         DEVICE int32 [B], or NULL: an array of the handle, read with vfik_waited_host.
 * Deliberately out of scope: an arm that never gets room waits until the time-out and keeps pending up; two arms that both yield can wait
 * for each other -- `yields` is the remedy: one arm of a pair yields, the other does not.  Taking a waiting arm out of pending after a
 * patience count belongs in the check kernels, next to the stall rule.
 * vfik_set_wait_rule may allocate (never under capture: VFIK_E_STATE), synchronises, and leaves vfik_launch_epoch and every launch
 * decision alone; the pointers are kept, not copied.  VFIK_E_ARG: min_clearance not finite, reserved != 0, a mask bit at or beyond L,
 * yields / clear_traj / pair_traj / waited no device pointer of its alignment (int32; the io type); VFIK_E_STATE: no coupling set.
 * vfik_waited_host copies waited[B] of the last timed move to the host and synchronises; VFIK_E_STATE without a rule or under capture. */
typedef struct vfik_wait_rule {
    double min_clearance;        /* finite */
    const int32_t* yields;       /* device [B] or NULL (every arm): only an arm with yields[b] != 0 ever waits */
    uint32_t mask[16];           /* own sphere i against partner sphere j; all zero = every pair */
    void* clear_traj;            /* device [n_checks][B] io dtype or NULL */
    int32_t* pair_traj;          /* device [n_checks][B] or NULL */
    int32_t* waited;             /* device [B] or NULL: the handle's own array, read with vfik_waited_host */
    int32_t reserved;            /* 0 */
} vfik_wait_rule;
size_t vfik_wait_rule_size(void);
int vfik_set_wait_rule(vfik_handle* h, const vfik_wait_rule* r);   /* NULL: off (the default) */
int vfik_waited_host(vfik_handle* h, int32_t* out /* host [B] */);

/* Whole-arm avoidance: link spheres that push their own joints.  The wait rule can only stop an arm; here the elbow gives way while the
 * hand keeps tracking its goal.  The reference's bridge keeps three command ports free for such extra joint commands, /bridge/mechanismcmd,
 * /bridge/xtra1cmd and /bridge/xtra2cmd (scripts/bridge:568-570,593-596): mixer channels 3..5, which the cycle kernels read from the
 * handle's ext buffer.  vfik_link_avoid computes such a command on the device.  For arm b, with the handle's link spheres
 * (link_i, c_i, r_i), i < L, rows first .. first + count - 1 of pts4[b][n_rep][4] = (Q_j, R_j) widened exactly, and the pair mask and the
 * NaN-row rule exactly as in vfik_link_clearance (bit j of mask[i]; a row that holds a NaN is no obstacle):
 *     P_i   = X_link_i(q_b) c_i               the public chain's frames, as vfik_link_points / vfik_link_clearance
 *     s_ij  = sqrt(|P_i - Q_j|^2)             from the coordinate differences, float64
 *     d_ij  = s_ij - r_i - R_j
 *     a_ij  = 1 - d_ij / d0                   the pair is ACTIVE iff a_ij > 0 (strict, so NaN never is) and s_ij > 0
 *     F_i   = gain * scale[b] * sum_j a_ij (P_i - Q_j) / s_ij          over the active pairs
 *     tau_k = sum over spheres with link_i > k of
 *               revolute joint k :  z_k . ((P_i - o_k) x F_i)
 *               prismatic joint k:  z_k . F_i
 *             z_k, o_k = third and fourth column of X_k, the frame of link k (joint k turns about / shifts along it)
 *     out[b][k] = (T) tau_k
 * The law is continuous at d_ij = d0, where the term is 0, and grows linearly into penetration; the only discontinuity is s_ij == 0, where
 * no direction exists: that pair contributes nothing.  A NaN anywhere in q[b] gives a row of ZEROS, not NaN (one NaN command would poison
 * qdot_out through a zero mixer weight); an arm with no active pair gets a row of zeros; every arm b < B is written on every call, so a
 * channel never keeps a stale push.
 *   d0     finite and > 0;  gain finite.
 *   scale  DEVICE [B] of the io dtype, or NULL for all ones: the per-arm priority tool, in the role yields has for the wait rule -- 0
 *          means this arm does not give way.
 *   out    DEVICE [B][n] of the io dtype, or NULL when a channel is named.
 *   channel  -1, or 3..5: the command is ALSO written into that channel of the handle's ext buffer (layout [4][B][n]), which must
 *          exist -- VFIK_E_STATE when neither vfik_set_ext_cmd nor vfik_set_avoid_rule has allocated it.  Channel 2 is the joint
 *          controller's and is refused.  The mixer weight of the channel is the caller's (vfik_params.mix_w, vfik_set_mixer_weights).
 * Asynchronous on the handle's stream, no allocation, ordered like vfik_link_clearance (the wait for outstanding vfik_submit_host tickets
 * included); no launch decision and no epoch moves; valid under stream capture.  [link_points; move_fields; link_avoid(channel = 4); step]
 * on one stream is the per-cycle form.
 * KNOWN COST: a handle whose ext buffer exists runs no lean cycle kernel (an ext command is a per-arm option), as after any
 * vfik_set_ext_cmd with a command.
 * VFIK_E_ARG: the window and mask refusals of vfik_link_clearance, d0 / gain as above, a channel outside {-1, 3, 4, 5}, neither out nor
 * a channel; VFIK_E_STATE: no spheres set, a channel without an ext buffer. */
int vfik_link_avoid(vfik_handle* h, const void* q, const void* pts4, int n_rep, int first, int count,
                    const uint32_t* mask /* host [L] or NULL */, double gain, double d0, const void* scale /* device [B] or NULL */,
                    void* out /* device [B][n] or NULL */, int channel);
/* The same with HOST arrays: q [B][n], pts4 [B][n_rep][4] and scale [B] (or NULL) doubles, rounded to the io dtype as
 * vfik_link_clearance_host rounds them; out [B][n] doubles receives the io-typed values, widened.  Copies, launches and synchronises; no
 * channel. */
int vfik_link_avoid_host(vfik_handle* h, const double* q, const double* pts4, int n_rep, int first, int count, const uint32_t* mask,
                         double gain, double d0, const double* scale, double* out);

/* The avoid rule: that command in front of every block of the timed moves.  State of the HANDLE like the wait rule, off by default; with
 * the rule off nothing changes -- the same launches, the same results.  It needs a coupling and goes when the coupling goes: a new sphere
 * list, vfik_set_coupling(h, NULL), vfik_set_chain.
 * While it is set, every block k of vfik_goto, vfik_follow, vfik_goto_js, vfik_follow_js and vfik_script enqueues avoid_kernel behind the
 * coupling's two launches (and behind the wait rule's, when there is one), on the block's INPUT row of joint angles against rows
 * first_rep .. first_rep + L - 1 of the coupling buffer; it writes the rule's channel and avoid_traj[k].  The command holds for the block's
 * `stride` cycles, as the coupling's repellers do.  When the move ends the channel is zeroed by one asynchronous memset on the stream: a
 * velocity push must not outlive the move, unlike a repeller's position.
 * The mixer weight of the channel is the caller's: vfik_params.mix_w or vfik_set_mixer_weights.  In vfik_script the weights of channels 4
 * and 5 come from the arm's own row (mix_frame / mix_posture carry 0..3), so channel 4 is the natural choice there.  A timed move under
 * the rule needs VFIK_F_MIXER (VFIK_E_STATE without).
 * vfik_set_avoid_rule is a setter like vfik_set_ext_cmd: it moves vfik_launch_epoch, may allocate the ext buffer (never under capture:
 * VFIK_E_STATE), zeroes the channel and synchronises; the pointers are kept, not copied.  While the rule is set, vfik_set_ext_cmd on the
 * rule's channel is refused (VFIK_E_STATE).  KNOWN COST as above: the ext buffer takes launches off the lean kernels.
 * VFIK_E_ARG: d0 not finite or <= 0, gain not finite, channel outside 3..5, reserved != 0, a mask bit at or beyond L, scale / avoid_traj
 * no device pointer aligned to the io type; VFIK_E_STATE: no coupling set. */
typedef struct vfik_avoid_rule {
    double gain, d0;
    int32_t channel, reserved;   /* 3..5; 0 */
    const void* scale;           /* device [B] io dtype or NULL (all ones) */
    uint32_t mask[16];           /* own sphere i against partner sphere j; all zero = every pair */
    void* avoid_traj;            /* device [n_checks][B][n] io dtype or NULL */
} vfik_avoid_rule;
size_t vfik_avoid_rule_size(void);
int vfik_set_avoid_rule(vfik_handle* h, const vfik_avoid_rule* r);   /* NULL: off (the default) */

/* Tracking-error estimator of scripts/vf (vf:349-428) for the batch: feed it, once per cycle, the tool
 * poses and field twists that vfik_step produced (device pointers pose[B][16], v6[B][6]); out[B][8] gets
 * vel_diff_angle, rot_diff_angle, ext_vel_mag_corr, ext_rot_mag_corr, cmd_vel_mag_corr, cmd_rot_mag_corr,
 * ext_int_diff, arm_tracking (the /track_error bottle, vf:418-427); zeros until the 6th frame (vf:354).
 * Per-arm history (previous frame, last 4 commands) lives in the handle; vfik_track_reset clears it.
 * active[B] (device, may be NULL = every arm): the estimator sits inside vf's `if qInBottle` block (vf:312-313,349),
 * so an arm without fresh joint angles appends no frame and no command -- its history and its out row stay. */
int vfik_track_error(vfik_handle* h, const void* pose, const void* v6, void* out, const int32_t* active);
int vfik_track_reset(vfik_handle* h);

/* Field probe of scripts/vf (vf:469-503, /pose_in -> /vector_out, "for visualizing"): every arm's field set
 * evaluated at a pose handed in instead of the arm's forward kinematics; device pose[B][16] -> device
 * v6[B][6] = speedScale * scalars * normCart(sum) (vf:491-494).  Asynchronous on the handle's stream. */
int vfik_probe_field(vfik_handle* h, const void* pose, void* v6);

/* Distance monitor of scripts/monitor_distance (monitor_distance:76-84,148-167) for the batch: device
 * pose[B][16] (what vfik_step wrote to io->pose), device frames[B][max_objects][16] (the object frames of
 * /dmonitor/objectsIn, object_feeder:215-227,306-315; unused slots may hold anything finite), device
 * out[B][max_objects][2] = xyz distance, rotation angle in DEGREES -- one /dmonitor/distOut entry each
 * (monitor_distance:161-167).  Asynchronous on the handle's stream. */
int vfik_object_distances(vfik_handle* h, const void* pose, const void* frames, int max_objects, void* out);

/* The object frames of the distance monitor (scripts/monitor_distance keeps a dictionary id -> frame fed by
 * /dmonitor/objectsIn, monitor_distance:72,111-129; object_feeder:215-227,306-315) as device state of the handle, rewritten
 * only when a message changed them: host frames[n_arms][n_objects][16] doubles (row-major 4x4; unused slots: any finite
 * frame, e.g. identity) for the arms [first_arm, first_arm + n_arms).  n_objects (1..4096) is one number for the batch; a
 * call with another n_objects than the handle holds must cover every arm.  io->obj_dist of a cycle call then gets every
 * arm's distances to its objects, computed on the device from the pose of that cycle.  Arms gated off by io->active get no new
 * pose, hence no new distances either: their rows of obj_dist (like those of track_error) keep the caller's content (ABI 5; until
 * then they were computed from the arm's previous pose).  The device buffers behind io->track_error / io->obj_dist are allocated
 * at the first call that asks for them -- a host that CAPTURES vfik_step into a hipGraph makes one such call outside the capture
 * first (VFIK_E_STATE otherwise). */
int vfik_set_objects(vfik_handle* h, int first_arm, int n_arms, const double* frames, int n_objects);

/* CommandMixer.read's weighted sum on its own (command_mixer.py:78-82): device cmds[K][B][n],
 * host weights[K], device out[B][n].  Bit-exact with the reference's left-to-right sum. */
int vfik_mix(vfik_handle* h, const void* cmds, const double* weights, int K, void* out);

/* Device memory for hosts that do not bring their own allocator (torch tensors work as well). */
void* vfik_dev_alloc(vfik_handle* h, size_t bytes);
int vfik_dev_free(vfik_handle* h, void* p);
int vfik_memcpy_h2d(vfik_handle* h, void* dst_dev, const void* src_host, size_t bytes);
int vfik_memcpy_d2h(vfik_handle* h, void* dst_host, const void* src_dev, size_t bytes);

/* hipEvent timing of `steps` back-to-back vfik_step launches on the handle's stream, after
 * `warmup` untimed ones: total elapsed ms -> *ms_total.  (bench.py: kernel time on the stream the
 * kernel really runs on.) */
int vfik_time_steps(vfik_handle* h, const vfik_io* io, int warmup, int steps, float* ms_total);

/* Small batches -- what vfclik itself runs is a handful of arms, each with its vf, nullspace and debug process and the bridge's
 * mixer (scripts/vfclik:88-105).  Launches the eight-lanes-per-arm kernel serves (revolute chain of up to 7 joints; no tool or ONE tool,
 * and IK weights shared by the batch; goal + integer-order decay repellers; with or without the nullspace module, joint-limit task, mixer, limiter,
 * /control; outputs qdot_out, qdot_vf, qdot_null, pose, pose_nt, qdist, status; no gate, no per-arm limits or weights) take it
 * instead of one lane per arm up to the batch size where the same-box A/B stops winning (profiles/r04_latency_small_*.txt;
 * DESIGN.md section 5.8): 4096 arms when the per-cycle rows are published; launches that ask for qdot_out alone (with or without the
 * nullspace module) stay on one lane per arm since round 4.  vfik_set_small_batch_kernel sets ONE threshold for all three cases (0 = never; the environment variable
 * VFIK_SUB8_MAX_BATCH does the same when the handle is created).  vfik_small_batch_launches: how many launches took that kernel
 * so far. */
int vfik_set_small_batch_kernel(vfik_handle* h, int max_batch);
long vfik_small_batch_launches(vfik_handle* h);
/* Introspection for tests: the cycle-kernel instantiations the handle's launches took since the last call, each once, as
 * newline-terminated demangled names without namespace and parameter list (`cycle_kernel_x<float, 7, ...>`; the long chains'
 * non-lean object adds " [heavy]").  A host-stepped rollout may name two: its intermediate cycles and its last.  Writes them to
 * buf (len bytes, NUL included) and clears the record; returns the length of the list.  buf == NULL: the length alone, nothing
 * cleared.  VFIK_E_ARG when len is too small, VFIK_E_STATE when more than 16 distinct kernels were launched since the last call. */
int vfik_launched_kernels(vfik_handle* h, char* buf, int len);

/* introspection for tests / DESIGN.md: slots in use, bytes of device state */
int vfik_slots_in_use(vfik_handle* h);
/* Which field path the handle's current field sets select for a cycle launch (decided when they are packed, vfik_set_fields):
 * 1 = straight-line: every arm is goal + decay repellers with integer orders (what object_feeder sends for point obstacles,
 * object_feeder:317-334: order 5 throughout; since ABI 5 the orders may differ between obstacles and between arms, as in
 * old/README.old:75, `ObstacleP ... 0.05 20`, beside the feeder's own order-5 near-goal repeller -- vfik_mixed_orders); 2 = straight-line with an aux block: as 1, and arms may carry ONE funnel attractor and ONE hemisphere
 * repeller with integer decay orders -- the goalAndNormal scene (object_feeder:248-303: attractor + approach funnel + near-goal
 * repeller + obstacles) and a surface (ObstacleH, object_feeder:344-353);
 * 0 = general: anything else (further attractors, several funnels or hemispheres, fractional orders or orders >= 128), entry by entry. */
int vfik_field_path(vfik_handle* h);
/* 1 when every decay repeller of the batch carries the same safe distance and the same force -- what the object feeder sends
 * (0.001 and -10 for every point obstacle and for the near-goal repeller: object_feeder:301-302,323,331): on field path 1 the lean
 * launches then read one quad (x y z radius) per repeller instead of 24 bytes, the pair from the batch constants.  0 otherwise. */
int vfik_uniform_repellers(vfik_handle* h);
/* 1 when, on top of vfik_uniform_repellers, the batch's repellers have decay order 5 and no arm has more than one chunk of them (8 with
 * float32 I/O) -- goal + up to 8 point obstacles as the object feeder sends them (object_feeder:302,333): the lean launches
 * (q -> qdot_out) of a float32 handle of up to 7 joints, at one wave per SIMD, then run the kernel's one-chunk order-5 body, which reads
 * its 8 repeller planes without looking at the slots in use.  Same results either way.  0 otherwise: float64 I/O, longer chains, other
 * orders, more obstacles, or the environment variable VFIK_ONE_CHUNK=0 at vfik_create (tests, A/B).  Decided by vfik_set_fields. */
int vfik_one_chunk(vfik_handle* h);
/* ABI 5.  1 when the decay repellers of the batch have integer orders that are not all the same: lean and publishing-lean
 * single-cycle launches of chains without a tool / weights then read one order byte per repeller beside the compact image and stay
 * on field path 1 / 2 (a wave whose 64 arms agree slot by slot pays scalar control flow only; a wave with an odd arm per-lane
 * selects); every other launch of such a batch (rollouts, per-arm options) takes the general path.  0 otherwise -- also with the
 * environment variable VFIK_MIXED_ORDERS=0, which restores the behaviour of ABI 4 (differing orders -> field path 0). */
int vfik_mixed_orders(vfik_handle* h);
/* ABI 5.  A counter that moves with every call that can change what a cycle launch bakes in at enqueue time -- the kernel variant and
 * its scalar arguments: field path, uniform / compact / order-plane image, slots in use, flags, PLAIN or not, per-arm option buffers
 * (tool, weights, mixer state, external commands), the small-batch thresholds -- i.e. every vfik_set_* call, vfik_reset_state and
 * vfik_set_small_batch_kernel.  A host that CAPTURED vfik_step / vfik_rollout launches into a hipGraph compares the value at capture
 * with the current one before a replay: a graph captured under another epoch may launch a stale variant (e.g. the uniform-image
 * kernel after one arm's (safe distance, force) pair changed) and must be re-captured.  Data the launch reads through pointers that
 * stay (q, the field images' CONTENT, nullspace state, external commands once allocated) needs no re-capture; the epoch moves anyway:
 * it is conservative. */
long vfik_launch_epoch(vfik_handle* h);
/* ABI 5, introspection.  1 when the chain set by vfik_set_chain matches a Denavit-Hartenberg pattern the lean float32-I/O kernels (and
 * the eight-lanes-per-arm kernel of small batches, either I/O type) are built for -- for 7 joints the KUKA LWR 4+ (vfclik's default robot, scripts/vfclik:42): a = 0 on every link, alpha = +-pi/2 on six,
 * d = 0 on three; for 14 joints two of them in series; for 6 joints the arm of vfclik_amd/robots.py -- and launches may take the
 * variants in which those links cost no arithmetic (all-revolute chain; no tool or ONE tool for the batch; IK weights shared by the batch); 0 otherwise: every
 * chain runs, the general DH form is the fallback.  VFIK_DH_PATTERN=0 in the environment switches the specialisation off. */
int vfik_dh_pattern(vfik_handle* h);
size_t vfik_device_bytes(vfik_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* VFIK_H */
