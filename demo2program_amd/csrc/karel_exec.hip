// Karel program metrics on the device: parse each predicted token string, run it from every
// demonstration's first frame and compare the execution with the demonstration -- the
// check_correct_syntax / generate_program_output / compare_demo_and_execution trio of
// models/program_metrics.py (reference models/model_full.py:602-616,745-780,878-901) in one launch.
//
// The host code is the specification (karel_env/dsl.py parse / _exec / _exec_cond, karel_env/karel.py):
//  - parse: the first-matching-rule shift-reduce machine; accepted when the input is used up and one
//    symbol of any kind is left.  The rule that can fire is decided by the top-of-stack symbol alone
//    (no two rules end in the same symbol), so the rule order needs no scan;
//  - execution: the call counter n, checked on entry to every statement / condition node and between
//    the halves of a sequence, +1 for prog, stmt, the first half of a sequence, IF / IFELSE conditions
//    and once per REPEAT; actions and WHILE iterations add nothing;
//  - world: state[h, w, 16] booleans, Karel = first set bit of channels 0-3 in row-major order, the
//    marker count = first set channel of 5..15 (0 if none), markersPresent = any of channels 6..15.
//
// Layout: one workgroup per row, 16 waves.  Lane 0 parses the row into an LDS node table; then wave
// v runs demos v, v+16, ...  Each lane of a wave owns one grid cell (h*w <= 64) and keeps its 16
// channels as bits of a register; control flow, the call counter and Karel's position are
// wave-uniform (ballot + shuffle).  The call stack is an explicit LDS stack per wave.
//
// Every loop is bounded independently of the program: the parser by KX_PARSE_CAP(L) steps, the
// interpreter by KX_EXEC_CAP steps and KX_STACK_CAP frames (the call counter bounds a correct run far
// below both); a row that hits a cap fails and raises a status flag.
#include "common.h"

#define KX_WAVES 16
#define KX_L_MAX 128
#define KX_NODE_CAP (4 * KX_L_MAX + 8)
#define KX_STACK_CAP 256
#define KX_EXEC_CAP 8192
#define KX_MAX_FUNC_CALL 100
#define KX_VOCAB 50

// nonterminal symbols (terminals are the token ids 0..49, karel_env/dsl.py _TOKENS)
enum { S_PROG = 50, S_STMT, S_STMT_STMT, S_WHILE, S_REPEAT, S_ACTION, S_IF, S_IFELSE, S_COND, S_COND_WO_NOT, S_CSTE };
// node kinds; fields: PROG/STMT/COND/NOT a = child; SEQ a, b; IF a = cond, b = body; IFELSE a = cond,
// b = then, c = else; WHILE a = cond, b = body; REPEAT a = count, b = body; PERCEPT / ACTION a = index
enum { K_PROG = 1, K_STMT, K_SEQ, K_IF, K_IFELSE, K_WHILE, K_REPEAT, K_ACTION, K_COND, K_NOT, K_PERCEPT, K_CSTE };
// tokens
enum { T_DEF = 0, T_RUN = 1, T_MO = 2, T_MC = 3, T_MOVE = 4, T_PUT = 8, T_RO = 9, T_RC = 10, T_R0 = 11, T_R19 = 30,
       T_REPEAT = 31, T_CO = 32, T_CC = 33, T_IO = 34, T_IC = 35, T_EO = 36, T_EC = 37, T_IF = 38, T_IFELSE = 39,
       T_ELSE = 40, T_FRONT = 41, T_NOMARK = 45, T_NOT = 46, T_WO = 47, T_WC = 48, T_WHILE = 49 };

struct KxSet {
    int k, T, cs, u8;
    const void* frames;   // [B, k, T, h, w, cs]
    const int* len;       // [B, k]
};

struct KxArgs {
    int L, ld_tok, h, w, make_error, keep_failed, T_out, kk;
    const int* tokens;
    const int* p_len;
    const int* is_same;
    KxSet set[2];
    int* syntax;
    int* exec_len;
    int* is_correct;
    int* num_correct;
    int* calls;
    int* frames;
    float* execution;
    int* status;
};

struct KxNodes {
    unsigned short kind[KX_NODE_CAP], a[KX_NODE_CAP], b[KX_NODE_CAP], c[KX_NODE_CAP];
};

// ---- parser (one lane) ----------------------------------------------------------------------------
__device__ static int kx_new(KxNodes& t, int& nn, int kind, int a, int b, int c) {
    if (nn >= KX_NODE_CAP) return -1;
    t.kind[nn] = kind; t.a[nn] = a; t.b[nn] = b; t.c[nn] = c;
    return nn++;
}

// dsl.py _reduce_once: -> 1 reduced, 0 no rule matches, -1 node table full
__device__ static int kx_reduce(unsigned char* sym, unsigned short* val, int& sp, KxNodes& t, int& nn) {
    const int top = sym[sp - 1];
    int lhs = -1, n = 0, node = -1;
#define KX_IS(i, s) (sym[sp - (i)] == (s))
    if (top == T_MC) {
        if (sp >= 5 && KX_IS(5, T_DEF) && KX_IS(4, T_RUN) && KX_IS(3, T_MO) && KX_IS(2, S_STMT)) {
            lhs = S_PROG; n = 5; node = kx_new(t, nn, K_PROG, val[sp - 2], 0, 0);
        }
    } else if (top == S_WHILE || top == S_REPEAT || top == S_STMT_STMT || top == S_ACTION || top == S_IF ||
               top == S_IFELSE) {
        lhs = S_STMT; n = 1; node = kx_new(t, nn, K_STMT, val[sp - 1], 0, 0);
    } else if (top == S_STMT) {
        if (sp >= 2 && KX_IS(2, S_STMT)) {
            lhs = S_STMT_STMT; n = 2; node = kx_new(t, nn, K_SEQ, val[sp - 2], val[sp - 1], 0);
        }
    } else if (top == T_IC) {
        if (sp >= 7 && KX_IS(7, T_IF) && KX_IS(6, T_CO) && KX_IS(5, S_COND) && KX_IS(4, T_CC) && KX_IS(3, T_IO) &&
            KX_IS(2, S_STMT)) {
            lhs = S_IF; n = 7; node = kx_new(t, nn, K_IF, val[sp - 5], val[sp - 2], 0);
        }
    } else if (top == T_EC) {
        if (sp >= 11 && KX_IS(11, T_IFELSE) && KX_IS(10, T_CO) && KX_IS(9, S_COND) && KX_IS(8, T_CC) &&
            KX_IS(7, T_IO) && KX_IS(6, S_STMT) && KX_IS(5, T_IC) && KX_IS(4, T_ELSE) && KX_IS(3, T_EO) &&
            KX_IS(2, S_STMT)) {
            lhs = S_IFELSE; n = 11; node = kx_new(t, nn, K_IFELSE, val[sp - 9], val[sp - 6], val[sp - 2]);
        }
    } else if (top == T_WC) {
        if (sp >= 7 && KX_IS(7, T_WHILE) && KX_IS(6, T_CO) && KX_IS(5, S_COND) && KX_IS(4, T_CC) &&
            KX_IS(3, T_WO) && KX_IS(2, S_STMT)) {
            lhs = S_WHILE; n = 7; node = kx_new(t, nn, K_WHILE, val[sp - 5], val[sp - 2], 0);
        }
    } else if (top == T_RC) {
        if (sp >= 5 && KX_IS(5, T_REPEAT) && KX_IS(4, S_CSTE) && KX_IS(3, T_RO) && KX_IS(2, S_STMT)) {
            lhs = S_REPEAT; n = 5; node = kx_new(t, nn, K_REPEAT, t.a[val[sp - 4]], val[sp - 2], 0);
        }
    } else if (top == S_COND_WO_NOT) {
        lhs = S_COND; n = 1; node = kx_new(t, nn, K_COND, val[sp - 1], 0, 0);
    } else if (top == T_CC) {
        if (sp >= 4 && KX_IS(4, T_NOT) && KX_IS(3, T_CO) && KX_IS(2, S_COND)) {
            lhs = S_COND; n = 4; node = kx_new(t, nn, K_NOT, val[sp - 2], 0, 0);
        }
    } else if (top >= T_FRONT && top <= T_NOMARK) {
        lhs = S_COND_WO_NOT; n = 1; node = kx_new(t, nn, K_PERCEPT, top - T_FRONT, 0, 0);
    } else if (top >= T_MOVE && top <= T_PUT) {
        // tokens move, turnRight, turnLeft, pickMarker, putMarker -> action indices 0, 2, 1, 3, 4
        const int idx = top == T_MOVE ? 0 : top == T_MOVE + 1 ? 2 : top == T_MOVE + 2 ? 1 : top - T_MOVE;
        lhs = S_ACTION; n = 1; node = kx_new(t, nn, K_ACTION, idx, 0, 0);
    } else if (top >= T_R0 && top <= T_R19) {
        lhs = S_CSTE; n = 1; node = kx_new(t, nn, K_CSTE, top - T_R0, 0, 0);
    }
#undef KX_IS
    if (lhs < 0) return 0;
    if (node < 0) return -1;
    sp -= n;
    sym[sp] = (unsigned char)lhs;
    val[sp] = (unsigned short)node;
    ++sp;
    return 1;
}

// ---- world (one wave; lane = cell) ---------------------------------------------------------------
struct KxLoc {
    int found, cell, z, kb;
};

__device__ __forceinline__ KxLoc kx_locate(unsigned bits) {
    const unsigned long long m = __ballot((bits & 0xFu) != 0);
    KxLoc l;
    l.found = m != 0ull;
    l.cell = l.found ? __builtin_ctzll(m) : 0;
    l.kb = __shfl((int)bits, l.cell, 64);
    l.z = l.found ? __builtin_ctz((unsigned)l.kb & 0xFu) : 0;
    return l;
}

// cell towards heading z (0 N, 1 E, 2 S, 3 W) or -1 when off the board
__device__ __forceinline__ int kx_ahead(int cell, int z, int h, int w) {
    int y = cell / w, x = cell - (cell / w) * w;
    y += z == 0 ? -1 : (z == 2 ? 1 : 0);
    x += z == 1 ? 1 : (z == 3 ? -1 : 0);
    return (y < 0 || y >= h || x < 0 || x >= w) ? -1 : y * w + x;
}

__device__ __forceinline__ bool kx_clear(unsigned bits, const KxLoc& l, int turn, int h, int w) {
    const int nc = kx_ahead(l.cell, (l.z + turn) & 3, h, w);
    const int nb = __shfl((int)bits, nc < 0 ? 0 : nc, 64);
    return nc >= 0 && !(nb & 0x10);
}

// Karel_world.state_transition; false = the action failed (raised)
__device__ static bool kx_act(unsigned& bits, int lane, int a, int make_error, int h, int w) {
    const KxLoc l = kx_locate(bits);
    if (!l.found) return false;                       // get_location raises inside the action
    if (a == 0) {
        if (kx_clear(bits, l, 0, h, w)) {
            const int nc = kx_ahead(l.cell, l.z, h, w);
            if (lane == nc) bits = (bits & ~0xFu) | ((unsigned)l.kb & 0xFu);
            if (lane == l.cell) bits &= ~0xFu;
        } else {
            if (make_error) return false;
            if (lane == l.cell) bits = (bits & ~0xFu) | (1u << ((l.z + 2) & 3));
        }
    } else if (a == 1 || a == 2) {
        if (lane == l.cell) bits = (bits & ~0xFu) | (1u << ((l.z + (a == 1 ? 3 : 1)) & 3));
    } else {
        const unsigned m5 = ((unsigned)l.kb >> 5) & 0x7FFu;
        const int n = m5 ? __builtin_ctz(m5) : 0;
        int nn = n + (a == 3 ? -1 : 1);
        if (nn < 0 || nn > 9) {
            if (make_error) return false;
            nn = n;
        }
        if (lane == l.cell) bits = (bits & 0x1Fu) | (1u << (5 + nn));
    }
    return true;
}

// _exec_cond: -> 0 / 1 value, -1 failure (n > MAX_FUNC_CALL), -2 no Karel (the host raises)
__device__ static int kx_cond(const KxNodes& t, int node, int n, unsigned bits, int h, int w) {
    if (n > KX_MAX_FUNC_CALL) return -1;
    int neg = 0;
    for (int i = 0; i < KX_NODE_CAP && t.kind[node] != K_PERCEPT; ++i) {
        neg ^= t.kind[node] == K_NOT;
        node = min((int)t.a[node], KX_NODE_CAP - 1);      // (the grammar ends every condition chain in a percept)
    }
    const KxLoc l = kx_locate(bits);
    if (!l.found) return -2;
    const int p = t.a[node];
    int v;
    if (p <= 2) v = kx_clear(bits, l, p == 0 ? 0 : (p == 1 ? 3 : 1), h, w);
    else v = ((unsigned)l.kb & 0xFFC0u) ? (p == 3) : (p == 4);
    return v ^ neg;
}

__device__ __forceinline__ float kx_frame_val(const KxSet& s, long base, int c) {
    return s.u8 ? (float)((const unsigned char*)s.frames)[base + c] : ((const float*)s.frames)[base + c];
}

// ---- the launch -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(KX_WAVES * 64) karel_exec_kernel(KxArgs a) {
    __shared__ KxNodes t;
    __shared__ unsigned char p_sym[KX_L_MAX];
    __shared__ unsigned short p_val[KX_L_MAX];
    __shared__ unsigned stack[KX_WAVES][KX_STACK_CAP];
    __shared__ int s_root, s_run, s_exec, s_status, s_num[2];

    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hw = a.h * a.w;
    const bool same = a.is_same[b] != 0;

    if (threadIdx.x == 0) {
        int len = a.p_len[b];
        len = len < 0 ? 0 : (len > a.L ? a.L : len);
        int ok = 0, status = 0, sp = 0, nn = 0;
        if (!same && len > 0) {
            int pos = 0, reduced = 0;
            const int cap = 8 * a.L + 16;              // a string needs <= len shifts + 4*len reductions
            for (int step = 0;; ++step) {
                if (!(pos < len || sp != 1)) { ok = 1; break; }
                if (step >= cap) { status |= D2P_KX_PARSE_CAP; break; }
                if (reduced) {
                    reduced = 0;
                } else {
                    const int tok = a.tokens[(long)b * a.ld_tok + pos++];
                    if (tok < 0 || tok >= KX_VOCAB) break;
                    p_sym[sp] = (unsigned char)tok;
                    p_val[sp] = (unsigned short)tok;
                    ++sp;
                }
                const int r = kx_reduce(p_sym, p_val, sp, t, nn);
                if (r < 0) { status |= D2P_KX_PARSE_CAP; break; }
                reduced = r;
                if (!reduced && pos >= len) break;
            }
        }
        const int top = ok ? p_sym[0] : 0;
        a.syntax[b] = same ? 1 : ok;
        s_exec = !same && ok;
        s_run = ok && top >= S_PROG && top <= S_IFELSE;     // prog, stmt, stmt_stmt, while, repeat, action, if, ifelse
        s_root = ok ? p_val[0] : 0;
        s_status = status;
        s_num[0] = s_num[1] = 0;
    }
    __syncthreads();

    const bool executed = s_exec != 0, runnable = s_run != 0;
    const int root = s_root;
    unsigned* stk = stack[wave];
    for (int d = wave; d < a.kk; d += KX_WAVES) {
        const int si = d < a.set[0].k ? 0 : 1;
        const KxSet s = si ? a.set[1] : a.set[0];
        const int dd = si ? d - a.set[0].k : d;
        const long fstride = (long)hw * s.cs;
        const long f0 = ((long)b * s.k + dd) * s.T * fstride + (long)lane * s.cs;   // this lane's cell of frame 0
        const int dlen = s.len[(long)b * s.k + dd];
        float* ex = a.execution ? a.execution + ((long)b * a.kk + d) * a.T_out * hw * 16 + (long)lane * 16 : nullptr;
        int status = 0, n = 0, nframes = 0;
        bool ok = false, match = true;
        unsigned bits = 0;

        auto record = [&]() {
            const int f = nframes++;
            if (ex && f < a.T_out && lane < hw) {
                float4* o = (float4*)(ex + (long)f * hw * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    o[q] = make_float4((bits >> (4 * q)) & 1, (bits >> (4 * q + 1)) & 1, (bits >> (4 * q + 2)) & 1,
                                       (bits >> (4 * q + 3)) & 1);
            }
            if (match && f < s.T) {
                bool eq = true;
                if (lane < hw)
                    for (int c = 0; c < 16; ++c)
                        eq &= kx_frame_val(s, f0 + f * fstride, c) == (float)((bits >> c) & 1);
                match = __ballot(!eq) == 0ull;
            }
        };

        if (executed) {
            if (lane < hw)
                for (int c = 0; c < 16; ++c) bits |= (kx_frame_val(s, f0, c) != 0.f ? 1u : 0u) << c;
            if (__ballot((bits & 0xFu) != 0) == 0ull) status |= D2P_KX_NO_KAREL;
            record();
        }
        if (executed && runnable) {
            // _exec over an explicit stack.  Frames are pushed for SEQ (second half pending), WHILE and
            // REPEAT (entry = node | iteration << 16); every other node tail-calls its child.
            int cur = root, sp = 0, call = 1, done = 0;
            for (int step = 0; step < KX_EXEC_CAP; ++step) {
                if (call) {
                    if (n > KX_MAX_FUNC_CALL) { ok = false; call = 0; continue; }
                    const int kd = t.kind[cur];
                    if (kd == K_PROG || kd == K_STMT) {
                        ++n;
                        cur = t.a[cur];
                    } else if (kd == K_SEQ || kd == K_REPEAT) {
                        ++n;
                        if (kd == K_REPEAT && t.a[cur] == 0) { ok = true; call = 0; continue; }
                        if (sp >= KX_STACK_CAP) { status |= D2P_KX_EXEC_CAP; break; }
                        stk[sp++] = (unsigned)cur | (kd == K_REPEAT ? 1u << 16 : 0u);
                        cur = kd == K_SEQ ? t.a[cur] : t.b[cur];
                    } else if (kd == K_IF || kd == K_IFELSE || kd == K_WHILE) {
                        if (kd != K_WHILE) ++n;
                        const int c = kx_cond(t, t.a[cur], n, bits, a.h, a.w);
                        if (c == -2) { status |= D2P_KX_COND_NO_KAREL; break; }
                        if (c < 0) { ok = false; call = 0; continue; }
                        if (kd == K_IFELSE) {
                            cur = c ? t.b[cur] : t.c[cur];
                        } else if (!c) {
                            ok = true; call = 0;
                        } else {
                            if (kd == K_WHILE) {
                                if (sp >= KX_STACK_CAP) { status |= D2P_KX_EXEC_CAP; break; }
                                stk[sp++] = (unsigned)cur;
                            }
                            cur = t.b[cur];
                        }
                    } else if (kd == K_ACTION) {
                        ok = kx_act(bits, lane, t.a[cur], a.make_error, a.h, a.w);
                        if (ok) record();
                        call = 0;
                    } else {
                        ok = false; call = 0;                    // not a statement (unreachable from a runnable root)
                    }
                } else {
                    if (sp == 0) { done = 1; break; }
                    const unsigned e = stk[sp - 1];
                    const int nd = (int)(e & 0xFFFFu), it = (int)(e >> 16), kd = t.kind[nd];
                    if (!ok) { --sp; continue; }
                    if (kd == K_SEQ) {
                        --sp;
                        if (n > KX_MAX_FUNC_CALL) { ok = false; continue; }
                        cur = t.b[nd]; call = 1;
                    } else if (kd == K_REPEAT) {
                        if (it < t.a[nd]) { stk[sp - 1] = (unsigned)nd | ((unsigned)(it + 1) << 16); cur = t.b[nd]; call = 1; }
                        else --sp;
                    } else {                                      // WHILE
                        const int c = kx_cond(t, t.a[nd], n, bits, a.h, a.w);
                        if (c == -2) { status |= D2P_KX_COND_NO_KAREL; break; }
                        if (c < 0) { --sp; ok = false; continue; }
                        if (c) { cur = t.b[nd]; call = 1; }
                        else --sp;
                    }
                }
            }
            if (!done) {
                if (!(status & (D2P_KX_EXEC_CAP | D2P_KX_COND_NO_KAREL))) status |= D2P_KX_EXEC_CAP;
                ok = false;
            }
        }

        const int elen = ok ? nframes : 0;
        bool correct = same;
        if (!same && elen == dlen) {
            // the rest of the T demo frames against the zero padding (all of them when nothing ran)
            bool eq = ok ? match : true;
            for (int f = ok ? (nframes < s.T ? nframes : s.T) : 0; eq && f < s.T; ++f) {
                bool z = true;
                if (lane < hw)
                    for (int c = 0; c < 16; ++c) z &= kx_frame_val(s, f0 + f * fstride, c) == 0.f;
                eq = __ballot(!z) == 0ull;
            }
            correct = eq;
        }
        if (ex && lane < hw) {
            const int keep = (ok || a.keep_failed) ? (nframes < a.T_out ? nframes : a.T_out) : 0;
            for (int f = keep; f < a.T_out; ++f) {
                float4* o = (float4*)(ex + (long)f * hw * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        if (lane == 0) {
            const long o = (long)b * a.kk + d;
            a.exec_len[o] = elen;
            a.is_correct[o] = correct;
            if (a.calls) a.calls[o] = n;
            if (a.frames) a.frames[o] = nframes;
            if (correct) atomicAdd(&s_num[si], 1);
            if (status) atomicOr(&s_status, status);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.num_correct[2 * b] = s_num[0];
        a.num_correct[2 * b + 1] = s_num[1];
        a.status[b] = s_status;
    }
}

static bool kx_geometry_ok(int B, int L, int h, int w, int depth) {
    return B > 0 && L > 0 && L <= KX_L_MAX && h > 0 && w > 0 && h * w <= 64 && depth == 16;
}

extern "C" size_t d2p_karel_exec_ws_bytes(int B, int L, int h, int w, int depth) {
    return kx_geometry_ok(B, L, h, w, depth) ? align_up((size_t)B * sizeof(int), 256) : 0;
}

extern "C" int d2p_karel_exec(int B, int L, const int* tokens, int ld_tok, const int* p_len, const int* is_same,
                              int h, int w, int depth, int flags,
                              int k, int T, const void* frames, int cs, const int* demo_len,
                              int k2, int T2, const void* frames2, int cs2, const int* demo2_len,
                              int* syntax, int* exec_len, int* is_correct, int* num_correct,
                              int* calls, int* nframes, float* execution, int T_out,
                              void* ws, size_t ws_bytes, d2p_stream_t stream) {
    D2P_REQUIRE(kx_geometry_ok(B, L, h, w, depth), D2P_EINVAL,
                "karel_exec: unsupported geometry B=%d L=%d h=%d w=%d depth=%d (needs B > 0, 0 < L <= %d, "
                "h*w <= 64, depth 16)", B, L, h, w, depth, KX_L_MAX);
    D2P_REQUIRE(ld_tok >= L && k >= 0 && k2 >= 0 && k + k2 > 0 && T_out >= 0 && (flags & ~15) == 0, D2P_EINVAL,
                "karel_exec: bad sizes");
    D2P_REQUIRE(k == 0 || (T > 0 && cs >= 16 && frames && demo_len), D2P_EINVAL, "karel_exec: bad first demo set");
    D2P_REQUIRE(k2 == 0 || (T2 > 0 && cs2 >= 16 && frames2 && demo2_len), D2P_EINVAL,
                "karel_exec: bad second demo set");
    D2P_REQUIRE(tokens && p_len && is_same && syntax && exec_len && is_correct && num_correct, D2P_EINVAL,
                "karel_exec: null pointer");
    D2P_REQUIRE(T_out == 0 || execution, D2P_EINVAL, "karel_exec: T_out > 0 needs execution");
    D2P_REQUIRE(ws && ws_bytes >= d2p_karel_exec_ws_bytes(B, L, h, w, depth), D2P_EINVAL,
                "karel_exec: workspace too small");
    KxArgs a;
    a.L = L; a.ld_tok = ld_tok; a.h = h; a.w = w;
    a.make_error = flags & D2P_KX_MAKE_ERROR ? 1 : 0;
    a.keep_failed = flags & D2P_KX_KEEP_FAILED ? 1 : 0;
    a.T_out = execution ? T_out : 0;
    a.kk = k + k2;
    a.tokens = tokens; a.p_len = p_len; a.is_same = is_same;
    a.set[0] = KxSet{k, T, cs, flags & D2P_KX_U8 ? 1 : 0, frames, demo_len};
    a.set[1] = KxSet{k2, T2, cs2, flags & D2P_KX_U8_2 ? 1 : 0, frames2, demo2_len};
    a.syntax = syntax; a.exec_len = exec_len; a.is_correct = is_correct; a.num_correct = num_correct;
    a.calls = calls; a.frames = nframes; a.execution = execution; a.status = (int*)ws;
    hipLaunchKernelGGL(karel_exec_kernel, dim3(B), dim3(KX_WAVES * 64), 0, as_stream(stream), a);
    D2P_LAUNCH_CHECK("karel_exec");
    return D2P_OK;
}
