// Kernel selection as ONE table: which kernels a (shape, counts, level) gets for the u phase, the u-dependent Gram entries
// and the alpha phase of an outer iteration (deconvolution.py:206-221).  Pure host functions of the key -- no pointers, no
// context -- so that dmf_solver_create / enqueue_outer_iteration / dmf_update_alpha / dmf_solver_describe read the same answer
// (every launch of an outer iteration, the alpha kernel included, is the one the plan names: launch_alpha() takes the
// AlphaKind) and a CPU test can enumerate a grid of keys against a checked-in table (tests/golden/kernel_selection.tsv,
// dmf_select_describe).  The key is frozen when the solver is created: a later dmf_context_set_generic does not reach it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace dmf {

// ---- thresholds (each measured; the measurement is cited where the constant is used in dmf_select.hip)
constexpr int kSplitInnerSteps = 50;        // beyond this many inner steps the split u phase beats the one-launch row pass
constexpr int kSizingInnerSteps = 20;       // the inner-step count select_path and dmf_solver_create ask the row pass's plan at
constexpr int kCmI8MinNu = 5;               // wide row groups: k_cm_i8 from this many unknowns on
constexpr int kSplitMinNu = 7;              // k_u_phase_mfma: split form from this many unknowns on (5 with known types)
constexpr int kGramI8MinFp64Acc = 48;       // integer Gram route instead of k_gram_u from this many FP64 accumulators on
constexpr int kGramI8MinPairsNoKnown = 33;  // ... and without known types from this many unknown pairs on (8 unknowns)

struct ShapeKey {
    int64_t N = 0;
    int S = 0, n_c = 0, n_u = 0;
    int nd = 0;                // count digit planes of the problem's integer copies (0: none -- counts not integral,
                               // beyond 32639, more than 2048 samples, R_trunc outside [0, 1])
    int SD = 0;                // padded sample count of those copies
    bool x16 = false;          // the problem carries X16 (the row pass reads x = d v as u16 instead of V)
    bool rowpass_pair = true;  // k_rowpass_v2 may run two blocks per phase B (X16 form; same kernel name, same results)
    bool rowpass_defer_c = true;  // ... and phase C deferred (four waves, x_byte; same results)
    bool rowpass_bytes = true;    // ... from the problem's byte images where it has them (same results; not in the text)
    bool x_byte = false;       // every count of the problem, so every x, is at most 255
    int level = 0;             // kernel selection level (dmf_context_set_generic): 0 fastest .. 4
    bool d_f32_exact = false;  // every count survives a round trip through f32
    bool rtp_present = true;   // the padded copy of R_trunc exists (n_c > 0)
    unsigned v_align = 0;      // address of V modulo 16
    unsigned rtp_align = 0;    // address of the padded R_trunc modulo 16
    bool alpha_unit = true;    // the starting alpha lies inside [0, 1] (the fixed-point features of the integer kernels)
};

// what dmf_solver_create fixes for the life of a solver
struct PathSpec {
    int u_path = 2;  // fall-back u phase: 0 k_u_phase_mfma, 1 k_u_phase_gram, 2 k_u_step_direct
    bool use_gram_spec = false, use_gram_mfma = false, use_u_big = false;
    bool use_v2 = false, use_cm_i8 = false, use_gram_i8 = false, use_fused = false;
    bool supported = true;  // false: no kernel takes this shape (DMF_ERR_UNSUPPORTED)
};

enum class RowKind {
    RowpassV2,        // k_rowpass_v2: u phase + b_u in one launch
    CmI8InnerBu,      // k_cm_i8 + k_inner_bu (b_u rides with the inner iterations)
    CmI8InnerRows,    // k_cm_i8 + k_u_inner_rows
    RowpassFused,     // first generation: k_rowpass_fused (Gram inside)
    UPhaseBig,        // k_u_phase_big
    UPhaseMfmaSplit,  // k_u_phase_mfma (split) + k_u_inner_rows
    UPhaseMfma,       // k_u_phase_mfma
    UPhaseGram,       // k_u_phase_gram
    UStepDirect       // k_u_step_direct, one launch per inner step
};
enum class GramKind { InRowPass, I8, BuColsI8, GramU, GramMfma, Gram };
enum class AlphaKind { FrankWolfeRow16, FrankWolfe, PhaseRow16, PhaseLanes, Phase, PhaseDyn };

// what ONE outer iteration with n_iter2 inner steps launches
struct IterationPlan {
    RowKind row = RowKind::UStepDirect;
    GramKind gram = GramKind::Gram;
    AlphaKind alpha = AlphaKind::PhaseDyn;
};

PathSpec select_path(const ShapeKey& k);
IterationPlan plan_iteration(const ShapeKey& k, const PathSpec& s, int n_iter2, bool purity);
// "rowpass=... gram=... alpha=..." (what dmf_solver_describe reports and the parity tests assert)
int describe_plan(const ShapeKey& k, const IterationPlan& plan, int n_iter2, char* buf, size_t cap);
// the PathSpec behind a u phase that runs as a kernel of its own (dmf_update_u): no one-launch row pass, no integer Gram
PathSpec standalone_spec(PathSpec s);
// The u phase alone, with what its launcher launches (dmf_u_phase_describe).  standalone: the u phase of dmf_update_u
// instead of the solver's loop.  For the first-generation FP64 row kernels the text is the launcher's own plan
// (dmf_internal.h: "k_u_phase_mfma<2,3,vec,d16> split nw=2 grid=512 lds=6912 raise=0 blocks/wg=3"); for the second
// generation it is the rowpass= part of describe_plan followed by the launcher's plan (k_rowpass_v2: RowpassV2Plan, which
// names the schedule; k_cm_i8: CmI8Plan).
int describe_u_phase(const ShapeKey& k, const PathSpec& s, int n_iter2, bool purity, bool standalone, char* buf, size_t cap);

// ---- the streaming cost (cost_f_w, deconvolution.py:15-17; the kernels and the plan: dmf_kernels_stream.hip).  Like the
// table above a pure function of a key, read by the launch (launch_cost_plan), by what the hold-out error asks about it
// and by the describe string (dmf_cost_describe, dmf_problem_cost_describe), so the three cannot drift apart.
struct CostKey {
    int S = 0, n_c = 0, n_u = 0;
    bool d16 = false;         // a u16 copy of the counts (or of the hold-out weights) is there to be read
    int SD = 0;               // its padded row length
    unsigned v_align = 0;     // address of V modulo 16
    bool rtp_present = true;  // the padded copy of R_trunc exists (n_c > 0)
    int level = 0;            // kernel selection level (dmf_context_set_generic)
};
enum class CostKind {
    Cols,       // k_cost_cols<NKC,NU,D16>: one sample per lane
    Cols2,      // k_cost_cols2<NKC,NU,ODD>, NU 0..4: two samples per lane
    Cols2Wide,  // k_cost_cols2<NKC,NU,ODD>, NU 5..16
    Generic     // k_cost: any shape
};
struct CostPlan {
    CostKind kind = CostKind::Generic;
    int nkc = 0, nu = 0;        // template arguments of the column-resident kernels
    bool d16 = false;           // the kernel reads the u16 counts (never the f64 copy)
    bool odd = false;           // k_cost_cols2: S is odd (the lone lane)
    bool alpha_in_lds = false;  // k_cost: alpha staged in LDS
};
constexpr int kCostPartials = 1024;  // scratch of the cost kernels: one partial per workgroup
CostPlan cost_plan(const CostKey& k);
// "cost=k_cost_cols2<3,4,odd>", "cost=k_cost_cols<2,1,u16>", "cost=k_cost alpha=lds"
int describe_cost_plan(const CostPlan& plan, char* buf, size_t cap);

}  // namespace dmf
