// rk3d_analysis.h -- the bodies of the analysis entry points of both 3-D models (lbmpm_rk3d_* / lbmpm_rk3dcsf_*: integrals, change,
// clusters, cluster_props, morphology), once, as templates over the context.  Included at file scope by rk3d.hip and rk3d_csf.hip
// after the analyses' headers (rk3d_integrals.h .. rk3d_change.h), the model's loaders and its context struct.
//
// A context has the members `mem`, `steps`, `integ`, `chg`, `cl`, `cprops`, `morph` under these names, and next to it the model says,
// in a specialisation AnalysisModel<Ctx> of static functions and nothing more:
//
//   AnalysisView view(const Ctx *c)                    device, streams and the own planes inside the lattice (below)
//   int enter(const char *who, Ctx *c)                 the checks that come first, then the context's device is current
//   int fresh(const char *who, Ctx *c, Analysis a)     LBMPM_ERR_STATE when what analysis `a` reads is stale (after the checks of the
//                                                      caller's configuration)
//   int with_flow(Ctx *c, f), int with_phi(Ctx *c, f)  return f(loader): the cells' rho, u, phi (IntCell) / phi alone
//
// `who` is the calling C function: every message names it as it did before.  A sixth analysis is one template here and one line in
// each of the two files.
#pragma once
#include "dispatch.h"

namespace {

enum class Analysis { Integrals, Change, Clusters, ClusterProps, Morphology };

struct AnalysisView {
    int device;
    hipStream_t stream;             // the analyses' kernels and copies
    hipStream_t zero_stream;        // first-use allocations are zeroed on it
    unsigned nx, ny, planes;        // the own planes
    unsigned z0, nzg;               // the global z of the first own plane, the planes of the whole lattice
    unsigned plane_cells() const { return nx * ny; }
};

template <typename Ctx>
struct AnalysisModel;

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_integrals(const char *who, Ctx *c, double *out)
{
    { const int rc = M::enter(who, c); if (rc) return rc; }
    { const int rc = M::fresh(who, c, Analysis::Integrals); if (rc) return rc; }
    const AnalysisView v = M::view(c);
    { const int rc = integral_buffer<FlowCols>(c->mem, &c->integ, v.planes, v.plane_cells(), 1, v.zero_stream); if (rc) return rc; }
    return M::with_flow(c, [&](const auto &load) -> int {
        LBMPM_HIP_TRY(integrals_run(load, v.planes, v.plane_cells(), c->integ, out, v.stream));
        return LBMPM_OK;
    });
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_change_ready(const char *who, Ctx *c)
{
    { const int rc = M::enter(who, c); if (rc) return rc; }
    return M::fresh(who, c, Analysis::Change);
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_change_mark(const char *who, Ctx *c)
{
    { const int rc = analysis_change_ready(who, c); if (rc) return rc; }
    const AnalysisView v = M::view(c);
    return M::with_flow(c, [&](const auto &load) -> int { return change_mark(load, c->chg, c->steps, v.planes, v.plane_cells(), c->mem, v.stream); });
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_change(const char *who, Ctx *c, int remark, int64_t *steps_between, double *out)
{
    { const int rc = analysis_change_ready(who, c); if (rc) return rc; }
    const AnalysisView v = M::view(c);
    return M::with_flow(c, [&](const auto &load) -> int {
        return change_run(who, load, c->chg, remark, c->steps, steps_between, v.planes, v.plane_cells(), out, v.stream);
    });
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_clusters(const char *who, Ctx *c, const lbmpm_clusters_config *cfg, int64_t *count)
{
    { const int rc = M::enter(who, c); if (rc) return rc; }
    const AnalysisView v = M::view(c);
    double cut = 0.;
    ClGeom g{};
    { const int rc = clusters_configure(who, cfg, (unsigned long long)v.nx * v.ny * (unsigned long long)v.nzg, &cut, &g); if (rc) return rc; }
    { const int rc = M::fresh(who, c, Analysis::Clusters); if (rc) return rc; }
    g.nx = v.nx; g.ny = v.ny; g.planes = v.planes; g.plane_cells = g.nx * g.ny; g.n = g.planes * g.plane_cells;
    g.z0 = v.z0; g.base = g.z0 * g.plane_cells;
    return M::with_phi(c, [&](const auto &load) -> int { return clusters_label(load, c->cl, g, cut, c->steps, c->mem, v.zero_stream, v.stream, count); });
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_clusters_table(const char *who, Ctx *c, int64_t *out)
{
    const AnalysisView v = M::view(c);
    return clusters_table(who, c->cl, c->steps, v.device, v.stream, out);
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_clusters_labels(const char *who, Ctx *c, uint32_t *out)
{
    const AnalysisView v = M::view(c);
    return clusters_labels(who, c->cl, c->steps, v.device, v.stream, out);
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_clusters_faces(const char *who, Ctx *c, uint32_t *labels, uint8_t *classes)
{
    const AnalysisView v = M::view(c);
    return clusters_faces(who, c->cl, c->steps, v.device, v.stream, labels, classes);
}

// (cluster_props: a context without a current table has nothing to be stale against; clusters_current, inside, says LBMPM_ERR_STATE)
template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_cluster_props_face(const char *who, Ctx *c, uint8_t *classes)
{
    { const int rc = M::fresh(who, c, Analysis::ClusterProps); if (rc) return rc; }
    const AnalysisView v = M::view(c);
    return M::with_flow(c, [&](const auto &load) -> int {
        return cluster_props_face(who, load, c->cl, c->cprops, c->steps, v.device, c->mem, v.zero_stream, v.stream, classes);
    });
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_cluster_props(const char *who, Ctx *c, const uint8_t *below, const uint8_t *above, int64_t *out)
{
    { const int rc = M::fresh(who, c, Analysis::ClusterProps); if (rc) return rc; }
    const AnalysisView v = M::view(c);
    return M::with_flow(c, [&](const auto &load) -> int {
        return cluster_props_run(who, load, c->cl, c->cprops, c->steps, v.device, c->mem, v.zero_stream, v.stream, below, above, out);
    });
}

// the checks and the class array of both morphology entry points; then the context's device is the current one
template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_morphology_ready(const char *who, Ctx *c, const lbmpm_morphology_config *cfg, const AnalysisView &v, double *cut)
{
    { const int rc = M::enter(who, c); if (rc) return rc; }
    { const int rc = morphology_configure(who, cfg, (unsigned long long)(v.planes + 1u) * v.nx * v.ny, cut); if (rc) return rc; }
    { const int rc = M::fresh(who, c, Analysis::Morphology); if (rc) return rc; }
    return morphology_classes(c->mem, &c->morph, v.planes, v.plane_cells(), v.zero_stream);
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_morphology_face(const char *who, Ctx *c, const lbmpm_morphology_config *cfg, uint8_t *classes)
{
    const AnalysisView v = M::view(c);
    double cut = 0.;
    { const int rc = analysis_morphology_ready(who, c, cfg, v, &cut); if (rc) return rc; }
    return M::with_flow(c, [&](const auto &load) -> int { return morphology_face(load, c->morph, v.plane_cells(), cut, classes, v.stream); });
}

template <typename Ctx, typename M = AnalysisModel<Ctx>>
int analysis_morphology(const char *who, Ctx *c, const lbmpm_morphology_config *cfg, const uint8_t *above, double *out)
{
    const AnalysisView v = M::view(c);
    double cut = 0.;
    { const int rc = analysis_morphology_ready(who, c, cfg, v, &cut); if (rc) return rc; }
    return M::with_flow(c, [&](const auto &load) -> int { return morphology_run(who, load, c->morph, v.planes, v.nx, v.ny, cut, above, out, v.stream); });
}

}  // namespace
