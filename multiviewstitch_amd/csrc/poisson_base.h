// poisson_base.h — what poisson_band.hip needs of poisson.hip: the checks of a plain call with another depth limit and those of the
// density parameters, the cube of rule 2, the base stage (rules 1-8 at one depth, chi left in scratch; with a gain per row the splat
// of rule 16), the gains of rule 16, and the device forms of the plain and the density call without their checks.  The kernels stay
// where they are; these are host functions around PnRun.
#ifndef MVS_POISSON_BASE_H_
#define MVS_POISSON_BASE_H_
#include "stitch.h"
#include "poisson_rules.h"

// check_call of a PN_PLAIN call with depth_min allowed up to max_depth; before a device is needed
int poisson_check_plain(const PnCall& c, int max_depth, const void* out_a, int64_t cap_a, const void* out_b, int64_t cap_b);
// check_call's part for dparams and dinfo (rules 14-16); before a device is needed
int poisson_check_density(const char* fn, int64_t n, const mvs_poisson_density_params* dp, const void* dinfo);
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
    // gain_dev (may be NULL): s_p per row, rule 16's splat x = w * (n_a * s_p) instead of rule 5's
    int solve(const PnCall& c, const double* pts_dev, const double* nrm_dev, hipStream_t s, const double* gain_dev = nullptr);
};
// rule 16 for n rows whose rho_p is on the device: gain_dev[i] = s_p (0 for a row that is not used), *n_clamped the used rows cut at
// max_gain.  Synchronises s.
int poisson_gains(int64_t n, const double* pts_dev, const double* nrm_dev, const double* rho_dev, double rho_mean, double max_gain, double* gain_dev,
                  int32_t* n_clamped, hipStream_t s);
// mvs_poisson_reconstruct_dev after its checks; bv and bf set: the mesh goes into blocks sized once the counts are known (and vcap,
// fcap are only tested)
int poisson_plain_dev(const PnCall& c, const double* pts_dev, const double* nrm_dev, double* vertices_dev, int64_t vcap, int32_t* faces_dev,
                      int64_t fcap, Scratch* bv, Scratch* bf, hipStream_t s);
// mvs_poisson_reconstruct_density_dev after its checks (c.rules = PN_DENSITY); density_dev / bd may be NULL: no vertex density
int poisson_density_dev(const PnCall& c, const double* pts_dev, const double* nrm_dev, double* vertices_dev, double* density_dev, int64_t vcap,
                        int32_t* faces_dev, int64_t fcap, Scratch* bv, Scratch* bd, Scratch* bf, hipStream_t s);
#endif
