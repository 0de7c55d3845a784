// vfik_check_body.inc -- the check kernels of the timed moves (vfik_aux.hip, which describes them and includes this text twice): with
// VFIK_STALL 0 it defines check_kernel<T, JOINT, LIST> and script_kernel<T>, with VFIK_STALL 1 check_stall_kernel and script_stall_kernel, which
// take the handle's stall rule (StallArgs, vfik_kernel.h) as a second argument.  One text, two builds: STALL is a compile-time constant of the
// body, and every statement of the rule sits in an `if constexpr (STALL)`, so the kernels without the rule stay the device code they were
// (a body shared as an inlined function did not: its argument block is copied before it is read, and the instruction order moved).
#if VFIK_STALL
#define VFIK_CHECK_NAME check_stall_kernel
#define VFIK_SCRIPT_NAME script_stall_kernel
#define VFIK_STALL_PARAM , const StallArgs st
#define VFIK_STALL_LOCAL constexpr bool STALL = true;
#else
#define VFIK_CHECK_NAME check_kernel
#define VFIK_SCRIPT_NAME script_kernel
#define VFIK_STALL_PARAM
#define VFIK_STALL_LOCAL constexpr bool STALL = false; const StallArgs st{};   // (st: named by discarded statements only)
#endif

template <typename T, bool JOINT, bool LIST>
__global__ void __launch_bounds__(256) VFIK_CHECK_NAME(const CheckArgs g VFIK_STALL_PARAM) {
    VFIK_STALL_LOCAL
    const int b = (int)(blockIdx.x * 256 + threadIdx.x);
    bool under_way = false;
    if (b < g.B) {
        const bool ua = !g.active || g.active[b] != 0;
        const int row = JOINT ? g.n : 16;   // elements of a list's item
        const T* const way = static_cast<const T*>(g.way) + (long)b * g.W * row;
        T* const goal = static_cast<T*>(g.goal);
        const long Qp = g.Bpad;   // quads per plane
        T* const rf = static_cast<T*>(g.ref) + (long)b * g.n;
        // the goal block's flag: a list asks for it here, beside next and len, so that the rule does not wait for it behind them
        bool present = false;
        if constexpr (LIST && !JOINT) present = goal[(3 * Qp + b) * 4] != (T)0;
        if (g.k < 0) {   // (uniform: the pass in front of block 0)
            bool in = ua;
            if constexpr (LIST) {
                int L = 0;
                while (L < g.W && way[(long)L * row] == way[(long)L * row]) ++L;
                for (int w = 0; w < g.W; ++w) g.reached[(long)b * g.W + w] = -1;
                g.next[b] = 0;
                g.len[b] = L;
                in = ua && L > 0;
            } else {
                g.arrived[b] = -1;
            }
            g.gate[b] = in ? 1 : 0;
            if constexpr (LIST && JOINT) {
                for (int i = 0; i < g.n; ++i) rf[i] = in ? way[i] : (T)__builtin_nan("");
            } else if constexpr (LIST) {
                if (in && present) follow_goal_store<T>(goal, b, Qp, way);
            }
            if constexpr (STALL) {
                stall_reset(st, b);
                st.stalled[b] = -1;
            }
            return;
        }
        int L = 1, nx;
        if constexpr (LIST) {
            L = g.len[b];
            nx = g.next[b];
        } else {
            nx = g.arrived[b] >= 0 ? 1 : 0;
        }
        const bool in = ua && L > 0;
        T* const qn = static_cast<T*>(g.q_now) + (long)b * g.n;
        bool stalled = false;   // (STALL: the arm has left the state machine)
        if constexpr (STALL) stalled = st.stalled[b] >= 0;
        if (g.gate[b] == 0) {
            const T* const qp = static_cast<const T*>(g.q_prev) + (long)b * g.n;
            for (int i = 0; i < g.n; ++i) qn[i] = qp[i];
            if constexpr (!JOINT) {
                if (g.dist_prev) {
                    T* const dn = static_cast<T*>(g.dist) + (long)b * 2;
                    const T* const dp = static_cast<const T*>(g.dist_prev) + (long)b * 2;
                    dn[0] = dp[0];
                    dn[1] = dp[1];
                }
            }
            if constexpr (LIST) {
                if (g.way_prev) g.way_now[b] = g.way_prev[b];
            }
        } else {
            if constexpr (LIST) {
                if (g.way_now) g.way_now[b] = nx < L ? nx : L - 1;
            }
            const bool last = !LIST || nx >= L - 1;
            bool there = false;
            double m0 = 0.0, m1 = 0.0;   // (STALL: the progress measure)
            if constexpr (JOINT) {
                T* const df = g.diff ? static_cast<T*>(g.diff) + (long)b * g.n : nullptr;
                bool ok = true;
                for (int i = 0; i < g.n; ++i) {
                    const double r = (double)rf[i], q = (double)qn[i], p = last ? g.prec[i] : g.via_prec[i];
                    ok = ok & ((r - p) <= q) & ((r + p) >= q);
                    if (df) df[i] = (T)(r - q);
                    if constexpr (STALL) {
                        if (p < __builtin_inf()) m0 = stall_max(m0, fabs(r - q));
                    }
                }
                there = nx < L && ok;
            } else if (nx < L) {
                const T* const dn = static_cast<const T*>(g.dist) + (long)b * 2;
                if constexpr (!LIST) present = goal[(3 * Qp + b) * 4] != (T)0;
                const double d = (double)dn[0];
                const double a = ((double)dn[1] * M_PI) / 180.0;
                there = present && d < (last ? g.prec[0] : g.via_prec[0]) && a < (last ? g.prec[1] : g.via_prec[1]);
                if constexpr (STALL) {
                    m0 = present ? d : __builtin_nan("");
                    m1 = present ? a : __builtin_nan("");
                }
            }
            if constexpr (STALL) there = there && !stalled;
            if (there) {
                const int cycle = (g.k + 1) * g.stride - 1;
                if constexpr (LIST) {
                    g.reached[(long)b * g.W + nx] = cycle;
                    ++nx;
                    g.next[b] = nx;
                    if (nx < L) {
                        const T* const nw = way + (long)nx * row;
                        if constexpr (JOINT) {
                            for (int i = 0; i < g.n; ++i) rf[i] = nw[i];
                        } else {
                            follow_goal_store<T>(goal, b, Qp, nw);
                        }
                        if constexpr (STALL) stall_reset(st, b);
                    }
                } else {
                    g.arrived[b] = cycle;
                    nx = 1;
                }
            } else if constexpr (STALL) {
                if (!stalled && nx < L) stalled = stall_step(st, b, JOINT, m0, m1, (g.k + 1) * g.stride - 1);
            }
        }
        if constexpr (STALL) {
            g.gate[b] = (in && !(g.hold && nx == L) && !(st.stop && stalled)) ? 1 : 0;
            under_way = in && nx < L && !stalled;
        } else {
            g.gate[b] = (in && !(g.hold && nx == L)) ? 1 : 0;
            under_way = in && nx < L;
        }
    } else if (g.k < 0) {
        return;
    }
    const int cnt = __popcll(__ballot(under_way));   // lanes at or beyond B count nothing
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(g.pending, cnt);
}

// ------------------------------------------------------------------------------------------------
// The check of a motion script (vfik_script): check_kernel<T, *, true>'s state machine over a list whose items are goal frames (kind 1, way16)
// or postures (kind 2, wayq) -- the pick-and-place script of the reference's README: set_ref_js to the home posture, a list of gotoFrame
// calls, set_ref_js again, and around each change of kind HandleBridge.cartesian_controller() / joint_controller() (handlers.py:189-211,
// 481-497), the bottle [1, 1, 0, 0] or [0, 0, 1, 0] to /bridge/weight.  len[b] = the leading items of kind 1 or 2.  The rule of a check is
// that of the kind of item min(next, len - 1): the Cartesian one on the block's distance row (an arm without a goal block never passes), or
// the joint one on the arm's row of `ref` -- which holds that posture as the caller sent it -- with diff = (T)(ref - q).  "Send" is the
// frame into the goal block (follow_goal_store, where the block is present), or the posture into `ref`, and the mixer quad of the item's
// kind into plane 0 of the arm's row of mixw: ONE 16-byte store, by the advancing lanes alone.  `ref` starts with NaN until the arm's
// first posture (no controller: channel 2 is the external command) and keeps the last posture over the frame items behind it.
// k < 0: reached, next, len, the gate, item 0, and plane 1 of mixw (w4 w5 max_vel -) from the handle's per-arm bridge state or the
// batch-wide values; an arm that takes no part gets a zero quad in plane 0 (it never runs).
// Everything else -- rows that repeat, way_now, one item per check, the gate of the next block, pending[k] -- is check_kernel's.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) VFIK_SCRIPT_NAME(const ScriptArgs s VFIK_STALL_PARAM) {
    VFIK_STALL_LOCAL
    typedef typename FollowQuad<T>::type Quad;
    const CheckArgs& g = s.c;
    const int b = (int)(blockIdx.x * 256 + threadIdx.x);
    bool under_way = false;
    if (b < g.B) {
        const bool ua = !g.active || g.active[b] != 0;
        const int* const kind = s.kind + (long)b * g.W;
        const T* const way16 = static_cast<const T*>(g.way) + (long)b * g.W * 16;
        const T* const wayq = static_cast<const T*>(s.wayq) + (long)b * g.W * g.n;
        T* const goal = static_cast<T*>(g.goal);
        const long Qp = g.Bpad;   // quads per plane
        T* const rf = static_cast<T*>(g.ref) + (long)b * g.n;
        Quad* const mq = static_cast<Quad*>(s.mixw) + b;
        const bool present = goal[(3 * Qp + b) * 4] != (T)0;
        const Quad mix_frame = {(T)s.mix[0][0], (T)s.mix[0][1], (T)s.mix[0][2], (T)s.mix[0][3]};
        const Quad mix_posture = {(T)s.mix[1][0], (T)s.mix[1][1], (T)s.mix[1][2], (T)s.mix[1][3]};
        if (g.k < 0) {   // (uniform: the pass in front of block 0)
            int L = 0;
            while (L < g.W && (kind[L] == VFIK_STEP_FRAME || kind[L] == VFIK_STEP_POSTURE)) ++L;
            for (int w = 0; w < g.W; ++w) g.reached[(long)b * g.W + w] = -1;
            g.next[b] = 0;
            g.len[b] = L;
            const bool in = ua && L > 0;
            g.gate[b] = in ? 1 : 0;
            const bool posture = in && kind[0] == VFIK_STEP_POSTURE;
            for (int i = 0; i < g.n; ++i) rf[i] = posture ? wayq[i] : (T)__builtin_nan("");
            if (in && !posture && present) follow_goal_store<T>(goal, b, Qp, way16);
            const Quad zero = {(T)0, (T)0, (T)0, (T)0};
            mq[0] = in ? (posture ? mix_posture : mix_frame) : zero;
            const Quad u = {(T)s.bridge_u[0], (T)s.bridge_u[1], (T)s.bridge_u[2], (T)0};
            mq[Qp] = s.bridge ? static_cast<const Quad*>(s.bridge)[Qp + b] : u;
            if constexpr (STALL) {
                stall_reset(st, b);
                st.stalled[b] = -1;
            }
            return;
        }
        const int L = g.len[b];
        int nx = g.next[b];
        const bool in = ua && L > 0;
        bool stalled = false;   // (STALL: the arm has left the state machine)
        if constexpr (STALL) stalled = st.stalled[b] >= 0;
        T* const qn = static_cast<T*>(g.q_now) + (long)b * g.n;
        T* const dn = static_cast<T*>(g.dist) + (long)b * 2;
        // the item this check is made against (an arm that ran has L > 0) and the one behind it: both kinds are asked for at once, and the
        // distance pair beside them, so that neither the rule nor the send waits for a load of its own behind next and len
        const int at = nx < L ? nx : (L > 0 ? L - 1 : 0);
        const int kd = kind[at], kn = kind[at + 1 < g.W ? at + 1 : at];
        const T d0 = dn[0], d1 = dn[1];
        if (g.gate[b] == 0) {
            const T* const qp = static_cast<const T*>(g.q_prev) + (long)b * g.n;
            for (int i = 0; i < g.n; ++i) qn[i] = qp[i];
            if (g.dist_prev) {
                const T* const dp = static_cast<const T*>(g.dist_prev) + (long)b * 2;
                dn[0] = dp[0];
                dn[1] = dp[1];
            }
            if (g.way_prev) g.way_now[b] = g.way_prev[b];
        } else {
            if (g.way_now) g.way_now[b] = at;
            const bool last = nx >= L - 1;
            bool there = false;
            double m0 = 0.0, m1 = 0.0;   // (STALL: the progress measure)
            if (kd == VFIK_STEP_POSTURE) {
                T* const df = g.diff ? static_cast<T*>(g.diff) + (long)b * g.n : nullptr;
                bool ok = true;
                for (int i = 0; i < g.n; ++i) {
                    const double r = (double)rf[i], q = (double)qn[i], p = last ? s.js_prec[i] : s.js_via_prec[i];
                    ok = ok & ((r - p) <= q) & ((r + p) >= q);
                    if (df) df[i] = (T)(r - q);
                    if constexpr (STALL) {
                        if (p < __builtin_inf()) m0 = stall_max(m0, fabs(r - q));
                    }
                }
                there = nx < L && ok;
            } else if (nx < L) {
                const double d = (double)d0;
                const double a = ((double)d1 * M_PI) / 180.0;
                there = present && d < (last ? g.prec[0] : g.via_prec[0]) && a < (last ? g.prec[1] : g.via_prec[1]);
                if constexpr (STALL) {
                    m0 = present ? d : __builtin_nan("");
                    m1 = present ? a : __builtin_nan("");
                }
            }
            if constexpr (STALL) {
                there = there && !stalled;
                if (!there && !stalled && nx < L) stalled = stall_step(st, b, kd == VFIK_STEP_POSTURE, m0, m1, (g.k + 1) * g.stride - 1);
            }
            if (there) {
                g.reached[(long)b * g.W + nx] = (g.k + 1) * g.stride - 1;
                ++nx;
                g.next[b] = nx;
                if (nx < L) {   // (nx = at + 1 < L <= W: kn is this item's kind)
                    if (kn == VFIK_STEP_POSTURE) {
                        const T* const nw = wayq + (long)nx * g.n;
                        for (int i = 0; i < g.n; ++i) rf[i] = nw[i];
                        mq[0] = mix_posture;
                    } else {
                        if (present) follow_goal_store<T>(goal, b, Qp, way16 + (long)nx * 16);
                        mq[0] = mix_frame;
                    }
                    if constexpr (STALL) stall_reset(st, b);
                }
            }
        }
        if constexpr (STALL) {
            g.gate[b] = (in && !(g.hold && nx == L) && !(st.stop && stalled)) ? 1 : 0;
            under_way = in && nx < L && !stalled;
        } else {
            g.gate[b] = (in && !(g.hold && nx == L)) ? 1 : 0;
            under_way = in && nx < L;
        }
    } else if (g.k < 0) {
        return;
    }
    const int cnt = __popcll(__ballot(under_way));   // lanes at or beyond B count nothing
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(g.pending, cnt);
}

#undef VFIK_CHECK_NAME
#undef VFIK_SCRIPT_NAME
#undef VFIK_STALL_PARAM
#undef VFIK_STALL_LOCAL
