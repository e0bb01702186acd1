/*
 * femshell_oracle_quad.c -- the element path of femshell_oracle.c evaluated in IEEE binary128 (__float128, libquadmath).
 *
 * TEST INFRASTRUCTURE ONLY, and only of the CPU tests and tools/gen_golden_truth.py: GPU tests read the fixture
 * tests/golden/element_truth.npz that the generator writes, never this library.
 *
 * The same source with one arithmetic type switched: femshell_oracle.c is included with FSO_QUAD set (see the comment
 * at its top).  The wrappers below take doubles, which binary128 holds exactly, and round each result once to double:
 * against an FP64 evaluation that errs by a few ulp the rounded truth is off by at most half an ulp per entry.
 * Built by `make -C oracle quad` with gcc and -lquadmath into libfemshell_oracle_quad.so; everything but the wrappers
 * has hidden visibility, so the library can sit in one process beside libfemshell_oracle.so.
 */
#define FSO_QUAD 1
#include "femshell_oracle.c"

#define FSOQ_API __attribute__((visibility("default")))

static void widen(int n, const double *in, fso_real *out)
{
    for (int i = 0; i < n; i++) out[i] = in[i];
}

static void narrow(int n, const fso_real *in, double *out)
{
    if (!out) return;
    for (int i = 0; i < n; i++) out[i] = (double)in[i];
}

FSOQ_API void fsoq_material_matrices(const fso_material *mat, double Dm[9], double Dp[9])
{
    fso_real Dmw[9], Dpw[9];
    fsoq_wide_material_matrices(mat, Dmw, Dpw);
    narrow(9, Dmw, Dm);
    narrow(9, Dpw, Dp);
}

/* the FP64 layout of fso_tri3_parts (femshell_oracle.h), whose name the include above has taken for the wide one */
struct fso_tri3_parts_fp64 {
    double trafo[9], transUV[6], dphi[6], area, Ke_m[36], Ke_p[81], K_local[324], K_global_nm[324];
};

/* as fso_element_tri3, every field of parts rounded once; parts has the header's FP64 layout and may be NULL */
FSOQ_API int fsoq_element_tri3(const double xyz[9], const fso_material *mat, double Ke[324],
                               struct fso_tri3_parts_fp64 *parts)
{
    fso_real X[9], Kw[324];
    fsoq_tri3_parts pw;
    widen(9, xyz, X);
    if (fsoq_wide_element_tri3(X, mat, Kw, &pw)) return -1;
    narrow(324, Kw, Ke);
    if (parts) {
        narrow(9, pw.trafo, parts->trafo);
        narrow(6, pw.transUV, parts->transUV);
        narrow(6, pw.dphi, parts->dphi);
        parts->area = (double)pw.area;
        narrow(36, pw.Ke_m, parts->Ke_m);
        narrow(81, pw.Ke_p, parts->Ke_p);
        narrow(324, pw.K_local, parts->K_local);
        narrow(324, pw.K_global_nm, parts->K_global_nm);
    }
    return 0;
}

/* as fso_element_quad4; trafo (3x3, rows = local axes, may be NULL) is the frame that function keeps to itself */
FSOQ_API int fsoq_element_quad4(const double xyz[12], const fso_material *mat, double Ke[576], double *Ke_m,
                                double *Ke_p, double *K_global_nm, double *trafo)
{
    fso_real X[12], Kw[576], Kmw[64], Kpw[144], Kgw[576];
    widen(12, xyz, X);
    if (fsoq_wide_element_quad4(X, mat, Kw, Kmw, Kpw, Kgw)) return -1;
    narrow(576, Kw, Ke);
    narrow(64, Kmw, Ke_m);
    narrow(144, Kpw, Ke_p);
    narrow(576, Kgw, K_global_nm);
    if (trafo) {
        fso_real T[9], loc[12], dphi[8], area;
        if (quad4_frame(X, T, loc, dphi, &area)) return -1;
        narrow(9, T, trafo);
    }
    return 0;
}
