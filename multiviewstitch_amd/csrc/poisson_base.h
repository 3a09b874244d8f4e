// poisson_base.h — what poisson_band.hip needs of poisson.hip: the checks of a plain call with another depth limit and those of the
// density parameters, the cube of rule 2, the base stage (rules 1-8 at one depth, chi left in scratch; with a gain per row the splat
// of rule 16), the scan between a count and a scatter kernel (PnScan), the fold of partials and the face count of rule 12, the sampling
// density of rules 14-17 over dense or block-stored node sums (PnDensitySums: the splat, rho_p, rho_mean, the gains; the vertex
// densities), the tail every call ends with (PnOut, poisson_finish), and the device forms of the plain and the density call without
// their checks.  The kernels stay in poisson.hip, once; these are host functions around them and around PnRun.
#ifndef MVS_POISSON_BASE_H_
#define MVS_POISSON_BASE_H_
#include "stitch.h"
#include "poisson_band_rules.h"

// check_call of a PN_PLAIN call with depth_min allowed up to max_depth; before a device is needed
int poisson_check_plain(const PnCall& c, int max_depth, const void* out_a, int64_t cap_a, const void* out_b, int64_t cap_b);
// check_call's part for dparams and dinfo (rules 14-16); before a device is needed
int poisson_check_density(const char* fn, int64_t n, const mvs_poisson_density_params* dp, const void* dinfo);
// check_call's part for sparams and sinfo (rule 19); before a device is needed
int poisson_check_screen(const char* fn, const mvs_poisson_screen_params* sp, const void* sinfo);
// rules 1-2: the origin and side of the cube and N.  c.info is zeroed and receives n_used and origin.  MVS_E_DEGENERATE as the plain call.
int poisson_cube(const PnCall& c, const double* pts_dev, const double* nrm_dev, hipStream_t s, double origin[3], double* side);
// The base stage: rules 1-8 at depth c.p->depth_min (the caller sets depth_min = depth_max), and one V-cycle past rule 8's criterion.  c.p and c.info outlive the object;
// c.info holds depth, h, origin, n_used, cycles and rel_residual.  chi stays valid, (2^depth + 1)^3 doubles, until the object goes.
struct PnBaseField {
    PnGrid g{};
    const double* chi = nullptr;
    int64_t bytes = 0;                    // what the stage holds from the pool, about
    void* run = nullptr;
    PnBaseField() = default;
    PnBaseField(const PnBaseField&) = delete;
    PnBaseField& operator=(const PnBaseField&) = delete;
    ~PnBaseField();
    // gain_dev (may be NULL): s_p per row, rule 16's splat x = w * (n_a * s_p) instead of rule 5's.  With c.sp and c.sinfo (rule 37)
    // chi is the screened field of rules 19-22, its solve too run one cycle past its criterion; c.sinfo describes it.
    int solve(const PnCall& c, const double* pts_dev, const double* nrm_dev, hipStream_t s, const double* gain_dev = nullptr);
};
// The scan between a count and a scatter kernel, for nb workgroups: the count kernel writes cnt, run() leaves base[b] = the survivors in
// the workgroups before b and base[nb] = all survivors.  bytes: what alloc took.
struct PnScan {
    Scratch cnt, base, local, tot, rbase;
    int64_t bytes = 0;
    int alloc(size_t nb, hipStream_t s);
    void run(int nb, hipStream_t s);
};
// *out_dev = the sum of n partials, by one workgroup in a fixed order (k_pn_fold)
void poisson_fold(const double* part_dev, int n, double* out_dev, hipStream_t s);
// A stencil row of rules 20 and 38 as the kernels keep it: the 27 entries in the offset order of rule 20, then the row sum.
constexpr int PN_SC_ROW = 28;
// k_sc_convert over `rows` rows: the 27 int64 sums of every row and their int64 sum become doubles in place
void poisson_screen_convert(int64_t rows, long long* tab_dev, hipStream_t s);
// rule 12's count: cnt_dev[workgroup] = the face items (of `items`, 12 per cube item of mask_dev) that hold a triangle
void poisson_face_count(const uint8_t* mask_dev, int64_t items, int32_t* cnt_dev, hipStream_t s);

// The int64 node sums of the density grid g (rule 14) as a call holds them: dense in node order (num == NULL), or 64 per stored block
// of the level behind the block table num of T entries per axis (rule 32: BdBlockSums).  The kernels are instantiated for either.
struct PnDensitySums {
    PnGrid g;
    const int32_t* num;
    int32_t T;
    long long* sums;
};
// Rules 14-16 for n rows once the sums are zero: the splat, rho_dev[i] = rho_p and gain_dev[i] = s_p (0 for a row that is not used),
// and mean, min, max and n_clamped of dinfo.  part: 24 bytes for each of 1024 workgroups on the device.  Synchronises s.
int poisson_density_rows(int64_t n, const double* pts_dev, const double* nrm_dev, const PnDensitySums& d, int64_t n_used, double max_gain,
                         double* rho_dev, double* gain_dev, Scratch& part, mvs_poisson_density_info* dinfo, hipStream_t s);
// rule 17 (34): out_dev[v] = the density at vertex v, NaN at a vertex that is not finite.  Synchronises s.
int poisson_vertex_density(int64_t nv, const double* vertices_dev, const PnDensitySums& d, double* out_dev, hipStream_t s);

// Where a call writes, on the device: the caller's arrays of vcap and fcap rows (density NULL: not wanted), or — bv set — blocks that
// are sized once the counts are known (bd NULL: no density).
struct PnOut {
    double *vertices, *density;
    int32_t* faces;
    int64_t vcap, fcap;
    Scratch *bv, *bd, *bf;
};
// The tail of every call once info holds the counts: the capacity test, the blocks sized, the scatter and the vertex densities.
template <class Run>
int poisson_finish(const char* fn, Run& run, const mvs_poisson_info& info, PnOut o) {
    int rc;
    const int64_t V = info.n_vertices, F = info.n_faces;
    if (V > o.vcap || F > o.fcap) return bad(fn, "a capacity is below the count (info holds n_vertices and n_faces)");
    if (o.bv) {
        if ((rc = o.bv->alloc(24 * (size_t)V)) || (rc = o.bf->alloc(12 * (size_t)F)) || (o.bd && (rc = o.bd->alloc(8 * (size_t)V)))) return rc;
        o.vertices = o.bv->as<double>();
        o.faces = o.bf->as<int32_t>();
        o.density = o.bd ? o.bd->as<double>() : nullptr;
    }
    if ((rc = run.scatter(o.vertices, o.faces))) return rc;
    return run.vertex_density(o.vertices, o.density);
}
// mvs_poisson_reconstruct_dev or, with c.rules = PN_DENSITY, mvs_poisson_reconstruct_density_dev after its checks
int poisson_dense_dev(const PnCall& c, const double* pts_dev, const double* nrm_dev, PnOut o, hipStream_t s);
#endif
