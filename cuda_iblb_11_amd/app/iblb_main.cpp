// iblb_main.cpp — drop-in for the reference driver main.cu (binary `IBLB`, reference Makefile).
//
// Same 10 positional arguments (main.cu:284-296), the same derived parameters (main.cu:298-321),
// the same iteration sequence (cilia kinematics -> LB step -> IB, main.cu:817-934, here one
// iblb_step per iteration inside libiblb) and the same output files in the same text format:
//   <data>/Raw/<c_num>/<c_fraction>//SimLog.txt        run log            (main.cu:761-790, 1007-1060)
//   <data>//Flux/<..>-flux.dat                          it*t_scale  Q*x_scale (main.cu:612, 998-1004, 1030-1034)
//   <data>/Raw/<c_num>/<c_fraction>/<it>-fluid.dat      BigData only       (main.cu:940-971)
//   <data>/Cilia/<c_num>/<c_fraction>/<it>-cilia.dat    BigData only       (main.cu:975-994)
// Deviations: the data root is $IBLB_DATA_DIR (default "Data/") instead of the
// hard-coded Windows / ShARC paths (main.cu:591-594), its directories are created, and ShARC no
// longer selects device 3 (the device is LOCAL_RANK).
//
// Multi-GPU: launched one process per GPU (e.g. `torchrun --no-python --nproc-per-node N IBLB
// ...`), ranks split the lattice into x-slabs and exchange halos over RCCL inside libiblb; the
// RCCL id travels through a rendezvous file; rank 0 gathers the fields and writes every file.
//
// Extensions (environment): IBLB_PRECISION=f32 stores populations in float; IBLB_CHECKPOINT=<prefix>
// with IBLB_CHECKPOINT_EVERY=<iterations> writes <prefix>.rank<r> checkpoints; IBLB_RESTART=<prefix>
// resumes from them (flux file appended, not truncated; the checkpoints hold the observers below, iblb_save_checkpoint_ex,
// and an observer a checkpoint does not hold, as in a file of an earlier driver, is seeded as in a fresh run);
// IBLB_FIELDS_STRIDE=sx[,sy] (one GPU) also writes
// <it>-fields.dat beside every <it>-fluid.dat: every sx-th column and sy-th row through iblb_get_fields,
// x  y  u_x  u_y  vorticity (scaled like the fluid file), then the shear stress sxy in lattice units;
// IBLB_STATS=1 (one GPU) appends one line per output iteration to <..>-stats.dat beside the flux file, from one
// iblb_reduce_fields call over the whole lattice (lattice units, %.17g; BigData or not):
// it  sum(rho)  sum(rho u_x)  sum(rho u_y)  sum(KE)  max(u^2)  x  y  Ma = sqrt(max u^2)/0.57735  non-finite rho samples
// IBLB_TRACERS=nx_t,ny_t[,stride] (one GPU) seeds passive tracers (iblb_set_tracers) on a regular nx_t x ny_t grid,
// x = (i + 0.5) XDIM / nx_t, y = (j + 0.5) (YDIM - 1) / ny_t, tracer i * ny_t + j, updated every `stride` (default 1)
// iterations, and writes <it>-tracers.dat beside the fluid files at every output iteration (BigData or not): one line
// x  y  laps per tracer, lattice units, %.17g.  Checkpoints hold the tracers: a restarted run goes on with them.
// IBLB_PARTICLES=D[,drift_y[,bottom[,top[,seed]]]] (needs IBLB_TRACERS) puts a motion model on that grid
// (iblb_set_tracer_model): the tracers also jitter with the diffusivity D >= 0 (lattice units), settle with the velocity
// drift_y (default 0) along y, and meet the bottom and the top wall as clamp|reflect|absorb says (default
// absorb,reflect); seed (default 0) selects the random numbers.  At every output iteration, beside <it>-tracers.dat
// (which keeps its format), <it>-fates.dat holds one line per tracer and <it>-deposits.dat one line per column (%.17g),
//   index  status  iteration  x  y          x  bottom  top
// status 0 alive, 1 at the bottom, 2 at the top, `iteration` the one at which the tracer deposited (-1 while alive);
// bottom and top the tracers deposited in that column.  No checkpoint holds the model or the fates: under IBLB_RESTART
// the model is set afresh on the restored tracers with every tracer alive.
// IBLB_PROBES=nx_p,ny_p[,stride] (one GPU) lets the context record time series (iblb_set_history) at a regular
// nx_p x ny_p grid of probes, x = (i + 0.5) XDIM / nx_p, y = (j + 0.5) (YDIM - 1) / ny_p, probe i * ny_p + j, one
// record every `stride` (default 1) iterations: u_x, u_y, and C as well with IBLB_SCALAR.  The ring holds
// INTERVAL/stride + 1 records, so none is overwritten between outputs; at every output iteration, before every
// checkpoint and at the end of the run the driver drains the new records and appends them to <..>-probes.dat beside
// the flux file, one line per record and probe, lattice units, %.17g:  it  p  x  y  u_x  u_y  [c]  with `it` the
// iterations done when the record was taken.  IBLB_PATHLINES=1 (needs IBLB_TRACERS) records the tracers instead, at
// their stride, and appends  it  p  x  y  laps  per record and tracer to <..>-paths.dat.  A context records one
// history: setting both is refused.  No checkpoint holds a history: a restarted run sets it afresh at the restart
// iteration and goes on appending to the same file.
// IBLB_AVERAGE=stride[,nbins[,sx[,sy]]] (one GPU) lets the context average rho, u_x, u_y, their squares and u_x u_y
// (iblb_set_average) on every sx-th column and sy-th row (default 1) of the whole lattice, one sample every `stride`
// iterations, sample m into bin m % nbins (default 1 bin).  At every output iteration after the run's first it writes
// <it>-mean.dat beside the fluid files (BigData or not), one line per bin and sample, lattice units, %.17g:
// bin  x  y  n  mean_rho  mean_ux  mean_uy  var_ux  var_uy  cov_uxuy   with mean = sum/n, var = sum_sq/n - mean^2,
// cov = sum_uxuy/n - mean_ux mean_uy; a blank line after each window row; a bin with n == 0 writes nothing.  It then
// calls iblb_reset_average: each file is the average over the preceding output interval (the first file: from the
// run's first iteration).  Checkpoints hold the averages: a restarted run goes on with its bins and counts.
// IBLB_SCALAR=tau[,stride[,sx[,sy]]] (one GPU) lets the context advect and diffuse a passive scalar (iblb_set_scalar,
// D = (tau - 0.5)/3, `stride` substeps every `stride` iterations, default 1) seeded C = 1 for y < YDIM/2 and 0 above,
// no flux through the walls, and writes <it>-scalar.dat beside the fluid files at every output iteration (BigData or
// not): one line  x  y  c  per sample of every sx-th column and sy-th row (default 1), lattice units, %.17g.
// Checkpoints hold the scalar with its source, uptake, ends and gauges and their totals: a restarted run goes on with
// them (the checkpoint's configuration wins over the environment's).  With IBLB_STATS=1 as well, one more iblb_reduce_fields
// call (IBLB_FIELD_C, _CUX, _CUY over the whole lattice) appends one line per output iteration to <..>-cstats.dat beside
// the flux file (lattice units, %.17g):  it  sum(C)  sum(C^2)  min C  max C  sum(C u_x)  sum(C u_y)
// IBLB_SCALAR_SOURCE=flux[,decay] (needs IBLB_SCALAR) gives that scalar a source (iblb_set_scalar_source): the amount
// `flux` of C enters every column through the bottom wall per substep, and C decays everywhere at the first-order
// rate `decay` per substep (default 0); both finite, decay >= 0.  Everything else about IBLB_SCALAR stays as it is;
// with both set, sum(C) in <..>-cstats.dat tends to flux XDIM / decay.
// IBLB_SCALAR_UPTAKE=k_bottom[,k_top] (needs IBLB_SCALAR) makes the walls absorb that scalar (iblb_set_scalar_uptake):
// every column loses k * C at the wall per substep through the bottom / the top wall (default 0); both finite and
// >= 0.  At every output iteration <it>-uptake.dat beside <it>-scalar.dat holds one line per column (%.17g),
//   x  total_bottom  total_top
// the net amount of C that entered the column through each wall since the run's first iteration (negative: absorbed).
// IBLB_SCALAR_ENDS=left,right[,value_left[,value_right]] (needs IBLB_SCALAR) opens that scalar's ends in x
// (iblb_set_scalar_ends): left and right in noflux|value|outflow, the values (finite, default 0) for the ends of kind
// `value`; the fluid stays periodic.  At every output iteration <it>-ends.dat beside <it>-scalar.dat holds one line
// per row (%.17g),
//   y  total_left  total_right
// the net amount of C that entered the row through each end since the run's first iteration (negative: it left).
// IBLB_SCALAR_STATIONS=x[,x...] and IBLB_SCALAR_LEVELS=y[,y...] (either or both; they need IBLB_SCALAR) gauge that
// scalar's transport (iblb_set_scalar_gauges): station x is the link between column x and the column to its right,
// level y the link between row y and row y + 1, both lists strictly ascending.  At every output iteration, beside
// <it>-scalar.dat (%.17g), <it>-stations.dat holds one line per row and <it>-levels.dat one line per column,
//   y  right_0  left_0  right_1  left_1 ...          x  up_0  down_0  up_1  down_1 ...
// the populations that crossed each link towards +x / -x and +y / -y, summed over the substeps since the run's first
// iteration: right - left and up - down are the net amounts.
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/iblb.h"

using namespace std;

namespace {

// main.cu:22-33
const double C_S_DRIVER = 0.577;  // the driver's C_S (the LB kernels use 0.57735)
const double l_0 = 0.000006;
const double t_0 = 0.067;
const unsigned int LENGTH = 96;
const unsigned int YDIM = 192;

double seconds() {
    struct timeval tv;
    gettimeofday(&tv, nullptr);
    return (double)tv.tv_sec + (double)tv.tv_usec / 1e6;
}

template <typename T>
std::string to_string_3(const T a_value, const int n = 3) {  // main.cu:255-261
    std::ostringstream out;
    out << std::setprecision(n) << a_value;
    return out.str();
}

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

std::string env_str(const char* name, const char* dflt) {
    const char* v = getenv(name);
    return v && *v ? std::string(v) : std::string(dflt);
}

void mkdirs(const std::string& path) {
    std::string cur;
    for (size_t i = 0; i < path.size(); ++i) {
        cur += path[i];
        if (path[i] == '/' && cur.size() > 1) mkdir(cur.c_str(), 0755);
    }
    if (!cur.empty() && cur.back() != '/') mkdir(cur.c_str(), 0755);
}

int die(iblb_ctx* c, int rc, const char* what) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, iblb_last_error(c) ? iblb_last_error(c) : "");
    return 1;
}

// RCCL id from rank 0 to the others through a file (written whole, then renamed into place)
bool rendezvous(int rank, char id[IBLB_UNIQUE_ID_BYTES], std::string& path) {
    path = env_str("IBLB_RDZV", "");
    if (path.empty())
        path = "/tmp/iblb_rdzv_" + env_str("TORCHELASTIC_RUN_ID", "run") + "_" + env_str("MASTER_PORT", "0");
    const time_t t_start = time(nullptr);
    if (rank == 0) {
        if (iblb_rccl_unique_id(id) != IBLB_OK) return false;
        const std::string tmp = path + ".tmp";
        FILE* f = fopen(tmp.c_str(), "wb");
        if (!f) return false;
        const bool ok = fwrite(id, 1, IBLB_UNIQUE_ID_BYTES, f) == IBLB_UNIQUE_ID_BYTES;
        fclose(f);
        return ok && rename(tmp.c_str(), path.c_str()) == 0;
    }
    for (int tries = 0; tries < 1200; ++tries) {  // up to 120 s
        struct stat st;
        if (stat(path.c_str(), &st) == 0 && st.st_mtime >= t_start - 30) {
            FILE* f = fopen(path.c_str(), "rb");
            if (f) {
                const size_t n = fread(id, 1, IBLB_UNIQUE_ID_BYTES, f);
                fclose(f);
                if (n == IBLB_UNIQUE_ID_BYTES) return true;
            }
        }
        usleep(100000);
    }
    return false;
}

}  // namespace

int main(int argc, char* argv[]) {
    //----------------------------INITIALISING---------------------------- (main.cu:265-321)
    unsigned int c_fraction = 1;
    unsigned int c_num = 6;
    double Re = 1.0;
    unsigned int XDIM = 288;
    unsigned int T = 100000;
    unsigned int T_pow = 1;
    float T_num = 1.0;
    unsigned int ITERATIONS = T;
    unsigned int P_num = 100;
    float I_pow = 1.0;
    unsigned int INTERVAL = 500;
    unsigned int c_space = 48;
    bool ShARC = 0;
    bool BigData = 0;

    const int world = env_int("WORLD_SIZE", 1), rank = env_int("RANK", 0);
    const bool lead = rank == 0;

    if (argc < 11) {
        if (lead) cout << "Too few arguments! " << argc - 1 << " entered of 10 required. " << endl;
        return 1;
    }
    stringstream arg;
    arg << argv[1] << ' ' << argv[2] << ' ' << argv[3] << ' ' << argv[4] << ' ' << argv[5] << ' ' << argv[6] << ' '
        << argv[7] << ' ' << argv[8] << ' ' << argv[9] << ' ' << argv[10];
    arg >> c_fraction >> c_num >> c_space >> Re >> T_num >> T_pow >> I_pow >> P_num >> ShARC >> BigData;

    XDIM = c_num * c_space;
    T = nearbyint(T_num * pow(10, T_pow));
    ITERATIONS = T * I_pow;
    if (P_num == 0 || ITERATIONS / P_num == 0) {  // the reference divides by zero here (main.cu:301, 938)
        if (lead) cout << "Output interval is zero: " << P_num << " data points for " << ITERATIONS << " iterations" << endl;
        return 1;
    }
    INTERVAL = ITERATIONS / P_num;

    if (XDIM < 2 * LENGTH) {
        if (lead)
            cout << "not enough cilia in simulation! Cilia spacing of " << c_space << " requires at least "
                 << 2 * LENGTH / c_space << " cilia" << endl;
        return 1;
    }

    // windowed field output (extension): stride of the samples, 0 = off
    int fsx = 0, fsy = 0;
    if (const char* fs = getenv("IBLB_FIELDS_STRIDE"); fs && *fs) {
        const int n = sscanf(fs, "%d,%d", &fsx, &fsy);
        if (n == 1) fsy = fsx;
        if (n < 1 || fsx < 1 || fsy < 1) {
            if (lead) cerr << "IBLB_FIELDS_STRIDE must be sx[,sy] with sx, sy >= 1, got " << fs << endl;
            return 2;
        }
        if (world > 1) {  // vorticity needs the neighbour slabs' velocity: a lone slab only (include/iblb.h)
            if (lead) cerr << "IBLB_FIELDS_STRIDE is not available under a launcher (WORLD_SIZE > 1): run on one GPU" << endl;
            return 2;
        }
    }

    // whole-lattice statistics at every output iteration (extension)
    const bool stats_on = env_int("IBLB_STATS", 0) != 0;
    if (stats_on && world > 1) {  // each rank would reduce its own slab only: combining them is not the driver's yet
        if (lead) cerr << "IBLB_STATS is not available under a launcher (WORLD_SIZE > 1): run on one GPU" << endl;
        return 2;
    }

    // passive tracers (extension): a regular grid of nx_t x ny_t, 0 = off
    int tr_nx = 0, tr_ny = 0, tr_stride = 1;
    if (const char* ts = getenv("IBLB_TRACERS"); ts && *ts) {
        char tail = 0;
        bool ok = sscanf(ts, "%d,%d,%d%c", &tr_nx, &tr_ny, &tr_stride, &tail) == 3;  // (a trailing character: 4)
        if (!ok) {
            tr_stride = 1;
            ok = sscanf(ts, "%d,%d%c", &tr_nx, &tr_ny, &tail) == 2;
        }
        if (!ok || tr_nx < 1 || tr_ny < 1 || tr_stride < 1 || (long long)tr_nx * tr_ny > 100000000LL) {
            if (lead) cerr << "IBLB_TRACERS must be nx_t,ny_t[,stride] with nx_t, ny_t, stride >= 1 and at most 1e8 tracers, got " << ts << endl;
            return 2;
        }
        if (world > 1) {  // a tracer's four cells may straddle slabs: a lone slab only (include/iblb.h)
            if (lead) cerr << "IBLB_TRACERS is not available under a launcher (WORLD_SIZE > 1): run on one GPU" << endl;
            return 2;
        }
    }

    // the history (extension): a regular grid of nx_p x ny_p probes, 0 = off, or the tracers' pathlines; one per context
    int pr_nx = 0, pr_ny = 0, pr_stride = 1;
    if (const char* ps = getenv("IBLB_PROBES"); ps && *ps) {
        char tail = 0;
        bool ok = sscanf(ps, "%d,%d,%d%c", &pr_nx, &pr_ny, &pr_stride, &tail) == 3;  // (a trailing character: 4)
        if (!ok) {
            pr_stride = 1;
            ok = sscanf(ps, "%d,%d%c", &pr_nx, &pr_ny, &tail) == 2;
        }
        if (!ok || pr_nx < 1 || pr_ny < 1 || pr_stride < 1 || (long long)pr_nx * pr_ny > 100000000LL) {
            if (lead) cerr << "IBLB_PROBES must be nx_p,ny_p[,stride] with nx_p, ny_p, stride >= 1 and at most 1e8 probes, got " << ps << endl;
            return 2;
        }
        if (world > 1) {  // a probe's four cells may straddle slabs: a lone slab only (include/iblb.h)
            if (lead) cerr << "IBLB_PROBES is not available under a launcher (WORLD_SIZE > 1): run on one GPU" << endl;
            return 2;
        }
    }
    const bool paths_on = env_int("IBLB_PATHLINES", 0) != 0;
    if (paths_on) {
        if (world > 1) {
            if (lead) cerr << "IBLB_PATHLINES is not available under a launcher (WORLD_SIZE > 1): run on one GPU" << endl;
            return 2;
        }
        if (tr_nx == 0) {
            if (lead) cerr << "IBLB_PATHLINES needs IBLB_TRACERS: the pathlines are the tracers'" << endl;
            return 2;
        }
        if (pr_nx > 0) {
            if (lead) cerr << "IBLB_PROBES and IBLB_PATHLINES are both set: a context records one history (iblb_set_history)" << endl;
            return 2;
        }
    }

    // the tracers' motion model (extension): a diffusivity, a settling velocity along y, a kind per wall and a seed
    bool pa_on = false;
    iblb_tracer_model pa_model{0., {0., 0.}, {IBLB_TRACER_WALL_ABSORB, IBLB_TRACER_WALL_REFLECT}, 0ull};
    if (const char* ps = getenv("IBLB_PARTICLES"); ps && *ps) {
        // one to five parts separated by commas, nothing else
        std::vector<std::string> parts(1);
        for (const char* p = ps; *p; ++p) {
            if (*p == ',') parts.emplace_back();
            else parts.back() += *p;
        }
        bool ok = parts.size() <= 5;
        for (size_t n = 0; ok && n < parts.size() && n < 2; ++n) {  // D >= 0 and drift_y, both finite
            const char* p = parts[n].c_str();
            char* end = nullptr;
            errno = 0;
            const double v = strtod(p, &end);
            ok = ((*p >= '0' && *p <= '9') || *p == '.' || *p == '+' || *p == '-') && end != p && *end == 0 &&
                 errno == 0 && std::isfinite(v) && (n == 1 || v >= 0.);
            (n == 0 ? pa_model.diffusivity : pa_model.drift[1]) = v;
        }
        for (size_t n = 2; ok && n < parts.size() && n < 4; ++n) {
            if (parts[n] == "clamp") pa_model.wall[n - 2] = IBLB_TRACER_WALL_CLAMP;
            else if (parts[n] == "reflect") pa_model.wall[n - 2] = IBLB_TRACER_WALL_REFLECT;
            else if (parts[n] == "absorb") pa_model.wall[n - 2] = IBLB_TRACER_WALL_ABSORB;
            else ok = false;
        }
        if (ok && parts.size() == 5) {
            const char* p = parts[4].c_str();
            char* end = nullptr;
            errno = 0;
            pa_model.seed = strtoull(p, &end, 10);
            ok = *p >= '0' && *p <= '9' && end != p && *end == 0 && errno == 0;
        }
        if (!ok) {
            if (lead)
                cerr << "IBLB_PARTICLES must be D[,drift_y[,bottom[,top[,seed]]]] with D >= 0 and drift_y finite, bottom "
                        "and top in clamp|reflect|absorb and seed a non-negative integer, got " << ps << endl;
            return 2;
        }
        if (world > 1) {  // the particles are the tracers: a lone slab only (include/iblb.h)
            if (lead) cerr << "IBLB_PARTICLES is not available under a launcher (WORLD_SIZE > 1): run on one GPU" << endl;
            return 2;
        }
        if (tr_nx == 0) {
            if (lead) cerr << "IBLB_PARTICLES needs IBLB_TRACERS: the particles are the tracers under a motion model" << endl;
            return 2;
        }
        pa_on = true;
    }

    // time- and phase-averaged fields (extension): sample stride, 0 = off
    int av_stride = 0, av_nbins = 1, av_sx = 1, av_sy = 1;
    if (const char* as = getenv("IBLB_AVERAGE"); as && *as) {
        // one to four integers >= 1 separated by commas, nothing else
        int* const dst[4] = {&av_stride, &av_nbins, &av_sx, &av_sy};
        bool ok = true;
        int n = 0;
        for (const char* p = as; ok; ++n) {
            char* end = nullptr;
            errno = 0;
            const long v = strtol(p, &end, 10);
            ok = n < 4 && *p >= '0' && *p <= '9' && errno == 0 && v >= 1 && v <= 1000000000L &&
                 (*end == ',' || *end == 0);
            if (!ok) break;
            *dst[n] = (int)v;
            if (*end == 0) {
                ++n;
                break;
            }
            p = end + 1;
        }
        if (!ok || n < 1) {
            if (lead) cerr << "IBLB_AVERAGE must be stride[,nbins[,sx[,sy]]] with every value >= 1, got " << as << endl;
            return 2;
        }
        if (world > 1) {  // averaging on the slabs of a group is not built: a lone slab only (include/iblb.h)
            if (lead) cerr << "IBLB_AVERAGE is not available under a launcher (WORLD_SIZE > 1): run on one GPU" << endl;
            return 2;
        }
    }

    // passive scalar (extension): relaxation time, 0 = off
    double sc_tau = 0.;
    int sc_stride = 1, sc_sx = 1, sc_sy = 1;
    if (const char* ss = getenv("IBLB_SCALAR"); ss && *ss) {
        // a number > 0.5, then up to three integers >= 1, separated by commas, nothing else
        int* const dst[3] = {&sc_stride, &sc_sx, &sc_sy};
        char* end = nullptr;
        errno = 0;
        sc_tau = strtod(ss, &end);
        bool ok = ((*ss >= '0' && *ss <= '9') || *ss == '.') && end != ss && errno == 0 && std::isfinite(sc_tau) &&
                  sc_tau > 0.5 && (*end == ',' || *end == 0);
        for (int n = 0; ok && *end == ','; ++n) {
            const char* p = end + 1;
            errno = 0;
            const long v = strtol(p, &end, 10);
            ok = n < 3 && *p >= '0' && *p <= '9' && errno == 0 && v >= 1 && v <= 1000000000L && (*end == ',' || *end == 0);
            if (ok) *dst[n] = (int)v;
        }
        if (!ok) {
            if (lead)
                cerr << "IBLB_SCALAR must be tau[,stride[,sx[,sy]]] with tau > 0.5 and every other value an integer >= 1, got "
                     << ss << endl;
            return 2;
        }
        if (world > 1) {  // the scalar on the slabs of a group is not built: a lone slab only (include/iblb.h)
            if (lead) cerr << "IBLB_SCALAR is not available under a launcher (WORLD_SIZE > 1): run on one GPU" << endl;
            return 2;
        }
    }

    // the scalar's source (extension): a uniform influx through the bottom wall and a bulk decay
    bool sc_source = false;
    double sc_flux = 0., sc_decay = 0.;
    if (const char* ss = getenv("IBLB_SCALAR_SOURCE"); ss && *ss) {
        // one or two finite numbers separated by a comma, nothing else; the second >= 0
        double* const dst[2] = {&sc_flux, &sc_decay};
        const char* p = ss;
        bool ok = true;
        for (int n = 0; ok; ++n) {
            char* end = nullptr;
            errno = 0;
            const double v = strtod(p, &end);
            ok = n < 2 && ((*p >= '0' && *p <= '9') || *p == '.' || *p == '-' || *p == '+') && end != p && errno == 0 &&
                 std::isfinite(v) && (n == 0 || v >= 0.) && (*end == ',' || *end == 0);
            if (!ok) break;
            *dst[n] = v;
            if (*end == 0) break;
            p = end + 1;
        }
        if (!ok) {
            if (lead)
                cerr << "IBLB_SCALAR_SOURCE must be flux[,decay], both finite and decay >= 0, got " << ss << endl;
            return 2;
        }
        if (!(sc_tau > 0.)) {
            if (lead) cerr << "IBLB_SCALAR_SOURCE needs IBLB_SCALAR: there is no scalar to feed" << endl;
            return 2;
        }
        sc_source = true;
    }

    // the scalar's uptake (extension): uniform first-order rates at the two no-flux walls
    bool sc_uptake = false;
    double sc_rate[2] = {0., 0.};
    if (const char* ss = getenv("IBLB_SCALAR_UPTAKE"); ss && *ss) {
        // one or two finite numbers >= 0 separated by a comma, nothing else
        const char* p = ss;
        bool ok = true;
        for (int n = 0; ok; ++n) {
            char* end = nullptr;
            errno = 0;
            const double v = strtod(p, &end);
            ok = n < 2 && ((*p >= '0' && *p <= '9') || *p == '.' || *p == '+') && end != p && errno == 0 &&
                 std::isfinite(v) && v >= 0. && (*end == ',' || *end == 0);
            if (!ok) break;
            sc_rate[n] = v;
            if (*end == 0) break;
            p = end + 1;
        }
        if (!ok) {
            if (lead)
                cerr << "IBLB_SCALAR_UPTAKE must be k_bottom[,k_top], both finite and >= 0, got " << ss << endl;
            return 2;
        }
        if (!(sc_tau > 0.)) {
            if (lead) cerr << "IBLB_SCALAR_UPTAKE needs IBLB_SCALAR: there is no scalar to absorb" << endl;
            return 2;
        }
        sc_uptake = true;
    }

    // the scalar's open ends in x (extension): a kind per end and a uniform value for an end of kind `value`
    bool sc_ends = false;
    int sc_end_kind[2] = {IBLB_SCALAR_END_NOFLUX, IBLB_SCALAR_END_NOFLUX};
    double sc_end_value[2] = {0., 0.};
    if (const char* ss = getenv("IBLB_SCALAR_ENDS"); ss && *ss) {
        // two kinds and at most two finite numbers, separated by commas, nothing else
        std::vector<std::string> parts(1);
        for (const char* p = ss; *p; ++p) {
            if (*p == ',') parts.emplace_back();
            else parts.back() += *p;
        }
        bool ok = parts.size() >= 2 && parts.size() <= 4;
        for (size_t n = 0; ok && n < 2; ++n) {
            if (parts[n] == "noflux") sc_end_kind[n] = IBLB_SCALAR_END_NOFLUX;
            else if (parts[n] == "value") sc_end_kind[n] = IBLB_SCALAR_END_VALUE;
            else if (parts[n] == "outflow") sc_end_kind[n] = IBLB_SCALAR_END_OUTFLOW;
            else ok = false;
        }
        for (size_t n = 2; ok && n < parts.size(); ++n) {
            const char* p = parts[n].c_str();
            char* end = nullptr;
            errno = 0;
            const double v = strtod(p, &end);
            ok = ((*p >= '0' && *p <= '9') || *p == '.' || *p == '+' || *p == '-') && end != p && *end == 0 &&
                 errno == 0 && std::isfinite(v);
            sc_end_value[n - 2] = v;
        }
        if (!ok) {
            if (lead)
                cerr << "IBLB_SCALAR_ENDS must be left,right[,value_left[,value_right]] with left and right in "
                        "noflux|value|outflow and finite values, got " << ss << endl;
            return 2;
        }
        if (!(sc_tau > 0.)) {
            if (lead) cerr << "IBLB_SCALAR_ENDS needs IBLB_SCALAR: there is no scalar to open" << endl;
            return 2;
        }
        sc_ends = true;
    }

    // the scalar's transport gauges (extension): lists of columns and of rows
    std::vector<int> sc_gauge[2];  // stations, levels
    const char* const sc_gauge_env[2] = {"IBLB_SCALAR_STATIONS", "IBLB_SCALAR_LEVELS"};
    for (int g = 0; g < 2; ++g) {
        const char* ss = getenv(sc_gauge_env[g]);
        if (!ss || !*ss) continue;
        // non-negative integers separated by commas, nothing else; the range is the library's to check
        bool ok = true;
        for (const char* p = ss; ok;) {
            char* end = nullptr;
            errno = 0;
            const long v = strtol(p, &end, 10);
            ok = *p >= '0' && *p <= '9' && end != p && errno == 0 && v <= 0x7fffffffL && (*end == ',' || *end == 0);
            if (!ok) break;
            sc_gauge[g].push_back((int)v);
            if (*end == 0) break;
            p = end + 1;
        }
        if (!ok) {
            if (lead) cerr << sc_gauge_env[g] << " must be a list of non-negative integers n[,n...], got " << ss << endl;
            return 2;
        }
        if (!(sc_tau > 0.)) {
            if (lead) cerr << sc_gauge_env[g] << " needs IBLB_SCALAR: there is no scalar to gauge" << endl;
            return 2;
        }
    }
    bool sc_gauges = !sc_gauge[0].empty() || !sc_gauge[1].empty();

    const double dx = 1. / LENGTH;
    const double dt = 1. / (T);
    const double SPEED = 0.8 * 1000 / T;
    const double t_scale = 1000. * dt * t_0;
    const double x_scale = 1000000. * dx * l_0;
    const double s_scale = x_scale / t_scale;
    const double TAU = (SPEED * LENGTH) / (Re * C_S_DRIVER * C_S_DRIVER) + 1. / 2.;
    const double TAU2 = 1. / (12. * (TAU - (1. / 2.))) + (1. / 2.);
    const double Ma = 1. * SPEED / C_S_DRIVER;

    time_t rawtime;
    struct tm* timeinfo;
    time(&rawtime);
    timeinfo = localtime(&rawtime);
    const std::string start_stamp = asctime(timeinfo);

    if (lead) {
        cout << start_stamp << endl;
        cout << "Initialising...\n";
    }

    const int p_step = T * c_fraction / c_num;
    const unsigned int Ns = LENGTH * c_num;
    const int size = XDIM * YDIM;

    //----------------------------CONTEXT (replaces main.cu:363-754)----------------------------
    iblb_config cfg;
    iblb_config_default(&cfg);
    cfg.nx = (int)XDIM;
    cfg.ny = (int)YDIM;
    cfg.tau = TAU;
    cfg.tau2 = TAU2;
    cfg.precision = env_str("IBLB_PRECISION", "f64") == "f32" ? IBLB_PREC_F32 : IBLB_PREC_F64;
    cfg.device = env_int("LOCAL_RANK", 0);
    cfg.max_points = (int)Ns;
    if (world > 1) {
        cfg.x_begin = (int)((long long)rank * XDIM / world);
        cfg.x_count = (int)((long long)(rank + 1) * XDIM / world) - cfg.x_begin;
    }
    iblb_ctx* ctx = nullptr;
    int rc = iblb_create(&cfg, &ctx);
    if (rc) return die(nullptr, rc, "iblb_create");
    if (world > 1) {
        char id[IBLB_UNIQUE_ID_BYTES];
        std::string rdzv;
        if (!rendezvous(rank, id, rdzv)) {
            fprintf(stderr, "rank %d: RCCL rendezvous through %s failed\n", rank, rdzv.c_str());
            return 1;
        }
        if ((rc = iblb_attach_rccl(ctx, id, world, rank))) return die(ctx, rc, "iblb_attach_rccl");
        if (lead) unlink(rdzv.c_str());  // every rank has joined the communicator
    }
    // rho = RHO_0, u = 0, force = 0, f = feq (main.cu:636-754)
    if ((rc = iblb_set_state(ctx, nullptr, nullptr, nullptr, nullptr))) return die(ctx, rc, "iblb_set_state");
    iblb_cilia cil{(int)c_num, (double)c_space, (int)T, p_step};
    if ((rc = iblb_set_cilia(ctx, &cil))) return die(ctx, rc, "iblb_set_cilia");

    const std::string ckpt = env_str("IBLB_CHECKPOINT", "");
    const int ckpt_every = env_int("IBLB_CHECKPOINT_EVERY", 0);
    const std::string restart = env_str("IBLB_RESTART", "");
    const std::string rank_sfx = ".rank" + std::to_string(rank);
    unsigned int it0 = 0;
    // The observers a restart's checkpoint held are in place after the load, with their totals, counts and schedules:
    // the file's configuration wins over the environment's, nothing of them is seeded or configured again, and the
    // output files go on from the restored state.  An observer the file does not hold is seeded as in a fresh run.
    bool tr_restored = false, av_restored = false, sc_restored = false;
    size_t tr_n = (size_t)tr_nx * tr_ny;
    iblb_window av_win{0, 0, ((int)XDIM - 1) / av_sx + 1, ((int)YDIM - 1) / av_sy + 1, av_sx, av_sy};
    if (!restart.empty()) {
        if ((rc = iblb_load_checkpoint(ctx, (restart + rank_sfx).c_str()))) return die(ctx, rc, "iblb_load_checkpoint");
        long long t = 0;
        iblb_get_step(ctx, &t);
        it0 = (unsigned int)t;
        long long n = 0;
        int stride = 0, nbins = 0;
        if ((rc = iblb_tracer_count(ctx, &n, &stride, nullptr))) return die(ctx, rc, "iblb_tracer_count");
        if (n > 0) {
            tr_restored = true;
            tr_n = (size_t)n;
            tr_stride = stride;
        }
        iblb_window w{};
        unsigned fields = 0, flags = 0;
        if ((rc = iblb_average_info(ctx, &w, &fields, &stride, &nbins, &flags, nullptr))) return die(ctx, rc, "iblb_average_info");
        if (fields) {
            if (fields != (IBLB_FIELD_RHO | IBLB_FIELD_UX | IBLB_FIELD_UY) || flags != (IBLB_AVG_SQ | IBLB_AVG_UXUY) ||
                w.x0 != 0 || w.y0 != 0) {
                if (lead) cerr << "IBLB_RESTART: the checkpoint's average is not one this driver writes" << endl;
                return 2;
            }
            av_restored = true;
            av_win = w;
            av_stride = stride;
            av_nbins = nbins;
            av_sx = w.sx;
            av_sy = w.sy;
        }
        iblb_scalar sk{};
        if ((rc = iblb_scalar_info(ctx, &sk, nullptr))) return die(ctx, rc, "iblb_scalar_info");
        if (sk.stride > 0) {
            sc_restored = true;
            sc_tau = sk.tau;
            sc_stride = sk.stride;
            unsigned present = 0;
            if ((rc = iblb_scalar_uptake_info(ctx, &present, nullptr))) return die(ctx, rc, "iblb_scalar_uptake_info");
            sc_uptake = present != 0;
            if ((rc = iblb_scalar_ends_info(ctx, nullptr, nullptr, &present, nullptr))) return die(ctx, rc, "iblb_scalar_ends_info");
            sc_ends = present != 0;
            int ng[2] = {0, 0};
            if ((rc = iblb_scalar_gauges_info(ctx, &ng[0], nullptr, &ng[1], nullptr, nullptr)))
                return die(ctx, rc, "iblb_scalar_gauges_info");
            for (int g = 0; g < 2; ++g) sc_gauge[g].assign((size_t)ng[g], 0);
            if ((rc = iblb_scalar_gauges_info(ctx, nullptr, sc_gauge[0].data(), nullptr, sc_gauge[1].data(), nullptr)))
                return die(ctx, rc, "iblb_scalar_gauges_info");
            sc_gauges = ng[0] > 0 || ng[1] > 0;
        }
    }
    // the tracer grid, seeded at the run's first iteration (a restarted run's too, unless its checkpoint held tracers)
    std::vector<double> tr_x(tr_n), tr_y(tr_n);
    std::vector<int> tr_laps(tr_n);
    if (tr_n > 0 && !tr_restored) {
        // y fastest, like the populations: neighbouring lanes of the update kernel read neighbouring rows
        for (int i = 0; i < tr_nx; i++)
            for (int j = 0; j < tr_ny; j++) {
                tr_x[(size_t)i * tr_ny + j] = (i + 0.5) * XDIM / tr_nx;
                tr_y[(size_t)i * tr_ny + j] = (j + 0.5) * (YDIM - 1) / tr_ny;
            }
        if ((rc = iblb_set_tracers(ctx, (long long)tr_n, tr_x.data(), tr_y.data(), tr_stride)))
            return die(ctx, rc, "iblb_set_tracers");
    }
    // the motion model on those tracers; no checkpoint holds it or the fates: a restarted run sets it afresh on the
    // tracers its checkpoint held, every one alive
    std::vector<int> pa_status(pa_on ? tr_n : 0);
    std::vector<long long> pa_hit(pa_on ? tr_n : 0), pa_dep(pa_on ? 2 * (size_t)XDIM : 0);
    if (pa_on && (rc = iblb_set_tracer_model(ctx, &pa_model, nullptr, nullptr))) return die(ctx, rc, "iblb_set_tracer_model");
    // averaged fields: rho, u_x, u_y with their squares and u_x u_y on every av_sx-th column and av_sy-th row,
    // from the run's first iteration (a restarted run's too, unless its checkpoint held averages: those go on, and
    // the run's first output iteration lies before the checkpoint)
    const size_t av_np = av_stride > 0 ? (size_t)av_win.nx * av_win.ny : 0;
    std::vector<double> av_sum(3 * av_np), av_sq(3 * av_np), av_xy(av_np);
    bool av_first = !av_restored;  // the first output iteration writes no mean file
    if (av_stride > 0 && !av_restored &&
        (rc = iblb_set_average(ctx, &av_win, IBLB_FIELD_RHO | IBLB_FIELD_UX | IBLB_FIELD_UY, av_stride, av_nbins,
                               IBLB_AVG_SQ | IBLB_AVG_UXUY)))
        return die(ctx, rc, "iblb_set_average");
    // the scalar: C = 1 in the lower half of the channel, 0 above, no flux through the walls, from the run's first
    // iteration (a restarted run's too, unless its checkpoint held a scalar: that one goes on as it was, with its
    // source, uptake, ends and gauges and their totals)
    iblb_window sc_win{0, 0, ((int)XDIM - 1) / sc_sx + 1, ((int)YDIM - 1) / sc_sy + 1, sc_sx, sc_sy};
    std::vector<double> sc_out(sc_tau > 0. ? (size_t)sc_win.nx * sc_win.ny : 0);
    std::vector<double> up_total[2];
    for (auto& v : up_total) v.assign(sc_uptake ? (size_t)XDIM : 0, 0.);
    std::vector<double> end_total[2];
    for (auto& v : end_total) v.assign(sc_ends ? (size_t)YDIM : 0, 0.);
    std::vector<double> gauge_total[4];  // right, left, up, down
    for (int g = 0; g < 4; ++g) gauge_total[g].assign(sc_gauge[g / 2].size() * (size_t)(g < 2 ? YDIM : XDIM), 0.);
    if (sc_tau > 0. && !sc_restored) {
        std::vector<double> c0((size_t)size);
        for (int j = 0; j < size; j++) c0[j] = (unsigned int)j / XDIM < YDIM / 2 ? 1. : 0.;
        iblb_scalar sk{sc_tau, sc_stride, {IBLB_SCALAR_WALL_NOFLUX, IBLB_SCALAR_WALL_NOFLUX}, {0., 0.}};
        if ((rc = iblb_set_scalar(ctx, &sk, c0.data(), nullptr))) return die(ctx, rc, "iblb_set_scalar");
        if (sc_source) {
            const std::vector<double> influx((size_t)XDIM, sc_flux);
            const iblb_scalar_source src{nullptr, sc_decay, {influx.data(), nullptr}, {nullptr, nullptr}};
            if ((rc = iblb_set_scalar_source(ctx, &src))) return die(ctx, rc, "iblb_set_scalar_source");
        }
        if (sc_uptake) {
            const std::vector<double> k0((size_t)XDIM, sc_rate[0]), k1((size_t)XDIM, sc_rate[1]);
            const iblb_scalar_uptake up{{k0.data(), k1.data()}};
            if ((rc = iblb_set_scalar_uptake(ctx, &up))) return die(ctx, rc, "iblb_set_scalar_uptake");
        }
        if (sc_ends) {
            // a value given for an end of another kind is not used
            const iblb_scalar_ends ends{{sc_end_kind[0], sc_end_kind[1]},
                                        {sc_end_kind[0] == IBLB_SCALAR_END_VALUE ? sc_end_value[0] : 0.,
                                         sc_end_kind[1] == IBLB_SCALAR_END_VALUE ? sc_end_value[1] : 0.},
                                        {nullptr, nullptr}};
            if ((rc = iblb_set_scalar_ends(ctx, &ends))) return die(ctx, rc, "iblb_set_scalar_ends");
        }
        if (sc_gauges) {
            const iblb_scalar_gauges ga{(int)sc_gauge[0].size(), sc_gauge[0].empty() ? nullptr : sc_gauge[0].data(),
                                        (int)sc_gauge[1].size(), sc_gauge[1].empty() ? nullptr : sc_gauge[1].data()};
            if ((rc = iblb_set_scalar_gauges(ctx, &ga))) return die(ctx, rc, "iblb_set_scalar_gauges");
        }
    }

    //----------------------------------------DEFINE DIRECTORIES---------------------------------- (main.cu:589-631)
    std::string output_data = env_str("IBLB_DATA_DIR", "Data/");
    if (output_data.back() != '/') output_data += '/';
    const std::string raw_data = output_data + "Raw/" + to_string(c_num) + "/" + to_string(c_fraction) + "/";
    const std::string cilia_data = output_data + "Cilia/" + to_string(c_num) + "/" + to_string(c_fraction) + "/";
    std::string outfile = cilia_data;
    const std::string flux = output_data + "/Flux/" + to_string(c_fraction) + "_" + to_string(c_num) + "_" +
                             to_string(c_space) + "_" + to_string_3(Re) + "_" + to_string_3(T_num) + "x" +
                             to_string_3(T_pow) + "-flux.dat";
    const std::string stats_path = flux.substr(0, flux.size() - strlen("-flux.dat")) + "-stats.dat";
    const std::string cstats_path = flux.substr(0, flux.size() - strlen("-flux.dat")) + "-cstats.dat";
    const std::string hist_path = flux.substr(0, flux.size() - strlen("-flux.dat")) + (paths_on ? "-paths.dat" : "-probes.dat");
    const std::string parameters = raw_data + "/SimLog.txt";

    ofstream fsA, fsB, fsC;
    if (lead) {
        mkdirs(raw_data);
        mkdirs(cilia_data);
        mkdirs(output_data + "/Flux/");
        if (restart.empty()) {
            fsB.open(flux.c_str(), ofstream::trunc);
            fsB.close();
            if (stats_on) {
                fsB.open(stats_path.c_str(), ofstream::trunc);
                fsB.close();
            }
            if (stats_on && sc_tau > 0.) {
                fsB.open(cstats_path.c_str(), ofstream::trunc);
                fsB.close();
            }
            if (pr_nx > 0 || paths_on) {
                fsB.open(hist_path.c_str(), ofstream::trunc);
                fsB.close();
            }
        }
        //-----------------------------------OUTPUT PARAMETERS----------------------------- (main.cu:761-790)
        fsC.open(parameters.c_str(), ofstream::trunc);
        fsC.close();
        fsC.open(parameters.c_str(), ofstream::app);
        fsC << start_stamp << endl;
        fsC << "Size: " << XDIM << "x" << YDIM << endl;
        fsC << "Iterations: " << ITERATIONS << endl;
        fsC << "Reynolds Number: " << Re << endl;
        fsC << "Relaxation times: " << TAU << ", " << TAU2 << endl;
        fsC << "Spatial step: " << dx * l_0 << "m" << endl;
        fsC << "Time step: " << dt * t_0 << "s" << endl;
        fsC << "Mach number: " << Ma << endl;
        fsC << "Phase Step: " << c_fraction << "/" << c_num << endl;
        if (BigData) fsC << "\nBig Data is ON" << endl;
        else fsC << "\nBig Data is OFF" << endl;
        if (ShARC) fsC << "Running on ShARC" << endl;
        else fsC << "Running on local GPU" << endl;
        cout << "Running Simulation...\n";
    }

    // the history, set at the run's first iteration (a restarted run's too: no checkpoint holds a history, so the
    // series goes on in the same file from the restart iteration).  The ring holds every record between two drains:
    // the driver drains it at every output iteration, before every checkpoint and at the end of the run
    const bool hist_on = pr_nx > 0 || paths_on;
    const size_t hi_n = paths_on ? tr_n : (size_t)pr_nx * pr_ny;
    const int hi_stride = paths_on ? tr_stride : pr_stride;
    const int hi_planes = paths_on ? 3 : (sc_tau > 0. ? 3 : 2);
    std::vector<double> pr_x(paths_on ? 0 : hi_n), pr_y(paths_on ? 0 : hi_n), hi_out;
    std::vector<long long> hi_it;
    long long hi_drained = 0;
    if (hist_on) {
        // y fastest, like the populations: neighbouring lanes of the record kernel read neighbouring rows
        for (int i = 0; i < pr_nx; i++)
            for (int j = 0; j < pr_ny; j++) {
                pr_x[(size_t)i * pr_ny + j] = (i + 0.5) * XDIM / pr_nx;
                pr_y[(size_t)i * pr_ny + j] = (j + 0.5) * (YDIM - 1) / pr_ny;
            }
        const unsigned hf = paths_on ? 0u : (IBLB_FIELD_UX | IBLB_FIELD_UY | (sc_tau > 0. ? IBLB_FIELD_C : 0u));
        if ((rc = iblb_set_history(ctx, paths_on ? 0 : (long long)hi_n, pr_x.data(), pr_y.data(), hf, hi_stride,
                                   (long long)(INTERVAL / hi_stride) + 1, paths_on ? IBLB_HIST_TRACERS : 0u)))
            return die(ctx, rc, "iblb_set_history");
    }
    // the records taken since the last drain, appended to the history's file:  it  p  x  y  ux  uy  [c]  per record
    // and probe, or  it  p  x  y  laps  per record and tracer; `it` is the record's iteration (iblb_get_step then)
    auto drain_history = [&]() -> int {
        long long recorded = 0;
        if ((rc = iblb_history_info(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, &recorded)))
            return die(ctx, rc, "iblb_history_info");
        const long long cnt = recorded - hi_drained;
        if (cnt <= 0) return 0;
        hi_out.resize((size_t)cnt * hi_planes * hi_n);
        hi_it.resize((size_t)cnt);
        if ((rc = iblb_get_history(ctx, hi_drained, cnt, hi_out.data(), hi_it.data()))) return die(ctx, rc, "iblb_get_history");
        FILE* fh = fopen(hist_path.c_str(), "a");
        if (!fh) {
            fprintf(stderr, "cannot write %s: %s\n", hist_path.c_str(), strerror(errno));
            return 1;
        }
        for (long long r = 0; r < cnt; r++) {
            const double* rec = hi_out.data() + (size_t)r * hi_planes * hi_n;
            for (size_t k = 0; k < hi_n; k++) {
                if (paths_on) {
                    fprintf(fh, "%lld\t%zu\t%.17g\t%.17g\t%d\n", hi_it[(size_t)r], k, rec[k], rec[hi_n + k], (int)rec[2 * hi_n + k]);
                } else {
                    fprintf(fh, "%lld\t%zu\t%.17g\t%.17g\t%.17g\t%.17g", hi_it[(size_t)r], k, pr_x[k], pr_y[k], rec[k], rec[hi_n + k]);
                    if (hi_planes == 3) fprintf(fh, "\t%.17g", rec[2 * hi_n + k]);
                    fputc('\n', fh);
                }
            }
        }
        fclose(fh);
        hi_drained = recorded;
        return 0;
    };

    std::vector<double> rho, u, fld;
    iblb_window fwin{0, 0, 1, 1, 1, 1};
    if (fsx > 0) {
        fwin.nx = ((int)XDIM - 1) / fsx + 1;
        fwin.ny = ((int)YDIM - 1) / fsy + 1;
        fwin.sx = fsx;
        fwin.sy = fsy;
        if (BigData) fld.resize(4 * (size_t)fwin.nx * fwin.ny);
    }
    std::vector<float> s, u_s;
    std::vector<int> epsilon;
    if (lead && BigData) {
        rho.resize(size);
        u.resize(2 * (size_t)size);
        s.resize(2 * Ns);
        u_s.resize(2 * Ns);
        epsilon.resize(Ns);
    }

    time_t start = seconds();  // time_t as in main.cu:815
    time_t p_runtime = 0;
    double Q = 0.;

    //--------------------------ITERATION LOOP----------------------------- (main.cu:817-1024)
    // iblb_step runs whole iterations; the loop stops at every iteration the reference writes
    // output after (it % INTERVAL == 0), at it == INTERVAL and at checkpoints.
    const char* ng = getenv("IBLB_NAN_GUARD");
    const bool nan_guard = !(ng && std::string(ng) == "0");
    bool nan_warned = false;
    unsigned int it = it0;
    while (it < ITERATIONS) {
        unsigned int next = (it / INTERVAL) * INTERVAL;  // next output iteration >= it
        if (next < it) next += INTERVAL;
        if (ckpt_every > 0 && !ckpt.empty()) {
            const unsigned int c = ((it / ckpt_every) + 1) * ckpt_every - 1;  // last iteration before a save
            if (c < next) next = c;
        }
        if (next >= ITERATIONS) next = ITERATIONS - 1;
        if ((rc = iblb_step(ctx, (int)(next - it + 1)))) return die(ctx, rc, "iblb_step");
        it = next;

        //----------------------------DATA OUTPUT------------------------------ (main.cu:938-1005)
        long long bad = 0;  // non-finite populations at this output iteration
        if (it % INTERVAL == 0) {
            // not in the reference (it writes NaN fields on): a diverged run is reported at the first
            // output iteration that sees it, on every rank (the count is collective); that iteration's
            // output is written as the reference writes it, then the run stops with status 3 —
            // unless IBLB_NAN_GUARD=0, which keeps the reference's behaviour (warn once, go on)
            if ((rc = iblb_count_nonfinite(ctx, &bad))) return die(ctx, rc, "iblb_count_nonfinite");
            if (bad > 0 && !nan_warned) {
                cerr << "IBLB: the run diverged: " << bad << " non-finite populations at iteration " << it
                     << (nan_guard ? " (this iteration's output written, further iterations skipped)"
                                   : " (IBLB_NAN_GUARD=0: the run goes on, as the reference's)")
                     << endl;
                nan_warned = true;
            }
            if (BigData) {
                if ((rc = iblb_gather_macro(ctx, 0, lead ? rho.data() : nullptr, lead ? u.data() : nullptr)))
                    return die(ctx, rc, "iblb_gather_macro");
                if (lead) {
                    outfile = raw_data + to_string(it) + "-fluid.dat";
                    fsA.open(outfile.c_str());
                    for (int j = 0; j < (int)(XDIM * YDIM); j++) {
                        int x = j % XDIM;
                        int y = (j - j % XDIM) / XDIM;
                        double ab = sqrt(u[0 * size + j] * u[0 * size + j] + u[1 * size + j] * u[1 * size + j]);
                        fsA << x * x_scale << "\t" << y * x_scale << "\t" << u[0 * size + j] * s_scale << "\t"
                            << u[1 * size + j] * s_scale << "\t" << ab * s_scale << "\t" << rho[j] << endl;
                        if (x == (int)XDIM - 1) fsA << endl;
                    }
                    fsA.close();
                    if (fsx > 0) {
                        if ((rc = iblb_get_fields(ctx, &fwin, IBLB_FIELD_UX | IBLB_FIELD_UY | IBLB_FIELD_VORT | IBLB_FIELD_SXY,
                                                  fld.data())))
                            return die(ctx, rc, "iblb_get_fields");
                        const size_t np = (size_t)fwin.nx * fwin.ny;
                        outfile = raw_data + to_string(it) + "-fields.dat";
                        fsA.open(outfile.c_str());
                        for (int j = 0; j < fwin.ny; j++) {
                            for (int i = 0; i < fwin.nx; i++) {
                                const size_t k = (size_t)j * fwin.nx + i;
                                fsA << i * fsx * x_scale << "\t" << j * fsy * x_scale << "\t" << fld[k] * s_scale << "\t"
                                    << fld[np + k] * s_scale << "\t" << fld[2 * np + k] * s_scale / x_scale << "\t"
                                    << fld[3 * np + k] << "\n";
                            }
                            fsA << "\n";
                        }
                        fsA.close();
                    }
                    if ((rc = iblb_get_lagrangian(ctx, s.data(), u_s.data(), epsilon.data())))
                        return die(ctx, rc, "iblb_get_lagrangian");
                    outfile = cilia_data + to_string(it) + "-cilia.dat";
                    fsA.open(outfile.c_str());
                    for (unsigned int k = 0; k < Ns; k++) {
                        fsA << s[2 * k + 0] * x_scale << "\t" << s[2 * k + 1] * x_scale << "\t" << u_s[2 * k + 0] * s_scale
                            << "\t" << u_s[2 * k + 1] * s_scale << "\t" << epsilon[k] << "\n";
                        if (k % 96 == 95 || s[2 * k + 0] > XDIM - 1 || s[2 * k + 0] < 1) fsA << "\n";
                    }
                    fsA.close();
                }
            }
            if (stats_on) {
                iblb_field_stats st[5];  // ascending bit order: rho, momx, momy, ke, usq
                if ((rc = iblb_reduce_fields(ctx, nullptr, IBLB_FIELD_RHO | IBLB_QTY_MOMX | IBLB_QTY_MOMY | IBLB_QTY_KE | IBLB_QTY_USQ,
                                             st, nullptr, nullptr)))
                    return die(ctx, rc, "iblb_reduce_fields");
                FILE* fs = fopen(stats_path.c_str(), "a");
                if (!fs) {
                    fprintf(stderr, "cannot append to %s: %s\n", stats_path.c_str(), strerror(errno));
                    return 1;
                }
                fprintf(fs, "%u\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%d\t%d\t%.17g\t%lld\n", it, st[0].sum, st[1].sum,
                        st[2].sum, st[3].sum, st[4].max, st[4].max_i, st[4].max_j, sqrt(st[4].max) / 0.57735,
                        st[0].nonfinite);
                fclose(fs);
            }
            if (stats_on && sc_tau > 0.) {
                iblb_field_stats st[3];  // ascending bit order: c, cux, cuy
                if ((rc = iblb_reduce_fields(ctx, nullptr, IBLB_FIELD_C | IBLB_FIELD_CUX | IBLB_FIELD_CUY, st, nullptr, nullptr)))
                    return die(ctx, rc, "iblb_reduce_fields");
                FILE* fs = fopen(cstats_path.c_str(), "a");
                if (!fs) {
                    fprintf(stderr, "cannot append to %s: %s\n", cstats_path.c_str(), strerror(errno));
                    return 1;
                }
                fprintf(fs, "%u\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\n", it, st[0].sum, st[0].sum_sq, st[0].min,
                        st[0].max, st[1].sum, st[2].sum);
                fclose(fs);
            }
            if (tr_n > 0) {
                if ((rc = iblb_get_tracers(ctx, tr_x.data(), tr_y.data(), tr_laps.data())))
                    return die(ctx, rc, "iblb_get_tracers");
                outfile = raw_data + to_string(it) + "-tracers.dat";
                FILE* ft = fopen(outfile.c_str(), "w");
                if (!ft) {
                    fprintf(stderr, "cannot write %s: %s\n", outfile.c_str(), strerror(errno));
                    return 1;
                }
                for (size_t k = 0; k < tr_n; k++) fprintf(ft, "%.17g\t%.17g\t%d\n", tr_x[k], tr_y[k], tr_laps[k]);
                fclose(ft);
            }
            if (pa_on) {  // (tr_x, tr_y: read just above)
                if ((rc = iblb_get_tracer_fates(ctx, pa_status.data(), pa_hit.data())))
                    return die(ctx, rc, "iblb_get_tracer_fates");
                if ((rc = iblb_get_tracer_deposits(ctx, pa_dep.data(), pa_dep.data() + XDIM)))
                    return die(ctx, rc, "iblb_get_tracer_deposits");
                outfile = raw_data + to_string(it) + "-fates.dat";
                FILE* ff = fopen(outfile.c_str(), "w");
                if (!ff) {
                    fprintf(stderr, "cannot write %s: %s\n", outfile.c_str(), strerror(errno));
                    return 1;
                }
                for (size_t k = 0; k < tr_n; k++)
                    fprintf(ff, "%zu\t%d\t%lld\t%.17g\t%.17g\n", k, pa_status[k], pa_hit[k], tr_x[k], tr_y[k]);
                fclose(ff);
                outfile = raw_data + to_string(it) + "-deposits.dat";
                FILE* fd = fopen(outfile.c_str(), "w");
                if (!fd) {
                    fprintf(stderr, "cannot write %s: %s\n", outfile.c_str(), strerror(errno));
                    return 1;
                }
                for (unsigned int i = 0; i < XDIM; i++) fprintf(fd, "%u\t%lld\t%lld\n", i, pa_dep[i], pa_dep[XDIM + i]);
                fclose(fd);
            }
            if (sc_tau > 0.) {
                if ((rc = iblb_get_scalar(ctx, &sc_win, sc_out.data()))) return die(ctx, rc, "iblb_get_scalar");
                outfile = raw_data + to_string(it) + "-scalar.dat";
                FILE* fc = fopen(outfile.c_str(), "w");
                if (!fc) {
                    fprintf(stderr, "cannot write %s: %s\n", outfile.c_str(), strerror(errno));
                    return 1;
                }
                for (int j = 0; j < sc_win.ny; j++)
                    for (int i = 0; i < sc_win.nx; i++)
                        fprintf(fc, "%d\t%d\t%.17g\n", i * sc_sx, j * sc_sy, sc_out[(size_t)j * sc_win.nx + i]);
                fclose(fc);
            }
            if (sc_uptake) {
                if ((rc = iblb_get_scalar_uptake(ctx, up_total[0].data(), up_total[1].data(), nullptr, nullptr, nullptr)))
                    return die(ctx, rc, "iblb_get_scalar_uptake");
                outfile = raw_data + to_string(it) + "-uptake.dat";
                FILE* fu = fopen(outfile.c_str(), "w");
                if (!fu) {
                    fprintf(stderr, "cannot write %s: %s\n", outfile.c_str(), strerror(errno));
                    return 1;
                }
                for (size_t i = 0; i < (size_t)XDIM; i++)
                    fprintf(fu, "%zu\t%.17g\t%.17g\n", i, up_total[0][i], up_total[1][i]);
                fclose(fu);
            }
            if (sc_ends) {
                if ((rc = iblb_get_scalar_ends(ctx, end_total[0].data(), end_total[1].data(), nullptr, nullptr, nullptr)))
                    return die(ctx, rc, "iblb_get_scalar_ends");
                outfile = raw_data + to_string(it) + "-ends.dat";
                FILE* fe = fopen(outfile.c_str(), "w");
                if (!fe) {
                    fprintf(stderr, "cannot write %s: %s\n", outfile.c_str(), strerror(errno));
                    return 1;
                }
                for (size_t j = 0; j < (size_t)YDIM; j++)
                    fprintf(fe, "%zu\t%.17g\t%.17g\n", j, end_total[0][j], end_total[1][j]);
                fclose(fe);
            }
            if (sc_gauges) {
                if ((rc = iblb_get_scalar_gauges(ctx, gauge_total[0].data(), gauge_total[1].data(), gauge_total[2].data(),
                                                 gauge_total[3].data(), nullptr)))
                    return die(ctx, rc, "iblb_get_scalar_gauges");
                // stations: one line per row; levels: one line per column; a pair of totals per gauge
                const char* const name[2] = {"-stations.dat", "-levels.dat"};
                for (int g = 0; g < 2; ++g) {
                    if (sc_gauge[g].empty()) continue;
                    const size_t len = g == 0 ? (size_t)YDIM : (size_t)XDIM;
                    outfile = raw_data + to_string(it) + name[g];
                    FILE* fg = fopen(outfile.c_str(), "w");
                    if (!fg) {
                        fprintf(stderr, "cannot write %s: %s\n", outfile.c_str(), strerror(errno));
                        return 1;
                    }
                    for (size_t j = 0; j < len; j++) {
                        fprintf(fg, "%zu", j);
                        for (size_t k = 0; k < sc_gauge[g].size(); k++)
                            fprintf(fg, "\t%.17g\t%.17g", gauge_total[2 * g][k * len + j], gauge_total[2 * g + 1][k * len + j]);
                        fprintf(fg, "\n");
                    }
                    fclose(fg);
                }
            }
            if (av_stride > 0 && !av_first) {
                outfile = raw_data + to_string(it) + "-mean.dat";
                FILE* fm = fopen(outfile.c_str(), "w");
                if (!fm) {
                    fprintf(stderr, "cannot write %s: %s\n", outfile.c_str(), strerror(errno));
                    return 1;
                }
                for (int b = 0; b < av_nbins; b++) {
                    long long n = 0;
                    if ((rc = iblb_get_average(ctx, b, av_sum.data(), av_sq.data(), av_xy.data(), &n)))
                        return die(ctx, rc, "iblb_get_average");
                    if (n == 0) continue;
                    const double dn = (double)n;
                    for (int j = 0; j < av_win.ny; j++) {
                        for (int i = 0; i < av_win.nx; i++) {
                            const size_t k = (size_t)j * av_win.nx + i;
                            const double mr = av_sum[k] / dn, mx = av_sum[av_np + k] / dn, my = av_sum[2 * av_np + k] / dn;
                            fprintf(fm, "%d\t%d\t%d\t%lld\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\t%.17g\n", b, i * av_sx, j * av_sy,
                                    n, mr, mx, my, av_sq[av_np + k] / dn - mx * mx, av_sq[2 * av_np + k] / dn - my * my,
                                    av_xy[k] / dn - mx * my);
                        }
                        fprintf(fm, "\n");
                    }
                }
                fclose(fm);
                if ((rc = iblb_reset_average(ctx))) return die(ctx, rc, "iblb_reset_average");
            }
            av_first = false;
            if (hist_on && (rc = drain_history())) return rc;
            if ((rc = iblb_get_flux(ctx, &Q))) return die(ctx, rc, "iblb_get_flux");
            if (lead) {
                fsB.open(flux.c_str(), ofstream::app);
                fsB << it * t_scale << "\t" << Q * x_scale << endl;
                fsB.close();
            }
            if (bad > 0 && nan_guard) {
                iblb_destroy(ctx);
                return 3;
            }
        }

        if (it == INTERVAL && lead) {  // main.cu:1007-1022
            time_t cycle = seconds();
            p_runtime = (cycle - start) * (ITERATIONS / INTERVAL);
            time_t p_end = rawtime + p_runtime;
            timeinfo = localtime(&p_end);
            cout << "\nCompletion time: " << asctime(timeinfo) << endl;
            fsC << "\nCompletion time: " << asctime(timeinfo) << endl;
            fsC.close();
        }

        if (ckpt_every > 0 && !ckpt.empty() && (it + 1) % ckpt_every == 0) {
            if (hist_on && (rc = drain_history())) return rc;  // no checkpoint holds the history: its file is complete up to here
            if ((rc = iblb_save_checkpoint_ex(ctx, (ckpt + rank_sfx).c_str(), IBLB_CKPT_OBSERVERS)))
                return die(ctx, rc, "iblb_save_checkpoint_ex");
        }
        ++it;
    }
    if (hist_on && (rc = drain_history())) return rc;  // the records since the last output iteration

    if ((rc = iblb_get_flux(ctx, &Q))) return die(ctx, rc, "iblb_get_flux");
    if (lead) {
        fsB.open(flux.c_str(), ofstream::app);
        fsB << it * t_scale << "\t" << Q * x_scale << endl;
        fsB.close();

        //--------------------------RUNTIME OUTPUT---------------------------------- (main.cu:1036-1060)
        double end = seconds();
        double runtime = end - start;
        int hours(0), mins(0);
        double secs(0.);
        if (runtime > 3600) hours = nearbyint(runtime / 3600 - 0.5);
        if (runtime > 60) mins = nearbyint((runtime - hours * 3600) / 60 - 0.5);
        secs = runtime - hours * 3600 - mins * 60;
        // fsC is still open (and this open fails) unless it == INTERVAL was reached, as in the reference
        fsC.open(parameters.c_str(), ofstream::app);
        fsC << "Total runtime: ";
        if (hours < 10) fsC << 0;
        fsC << hours << ":";
        if (mins < 10) fsC << 0;
        fsC << mins << ":";
        if (secs < 10) fsC << 0;
        fsC << secs << endl;
        fsC.close();
    }
    iblb_destroy(ctx);
    return 0;
}
