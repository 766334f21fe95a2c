// loads.cpp -- host side of the distributed loads (include/stan_host.h): the pressure faces of a node
// set, and BuildDistributedLoads, which reads the BoundaryCondition Types "Pressure", "BodyForce" and "Displacement" into
// the flat arrays stan_hip_load_vector_hex8 takes; and of the thermal loads (section 3.9): BuildThermalLoads reads the Types
// "Temperature" and "ThermalExpansion" into the arrays stan_hip_thermal_load_hex8 takes.  No counterpart in the reference,
// which ignores Types it does not know (Solver.cs:106, 138): a file with such BCs stays readable by it.
#include <algorithm>
#include <array>
#include <string>
#include <vector>

#include "../../include/stan_host.h"
#include "model.h"

namespace stan {
namespace {
// local nodes of the six faces in CHEXA order (xi-, xi+, eta-, eta+, zeta-, zeta+)
const int FACE_NODES[6][4] = {{0, 3, 4, 7}, {1, 2, 5, 6}, {0, 1, 4, 5}, {2, 3, 6, 7}, {0, 1, 2, 3}, {4, 5, 6, 7}};

struct Candidate {
    std::array<int32_t, 4> key;   // sorted distinct nodes, padded with -1
    int32_t elem;
    uint8_t face;
    double p;
};
}  // namespace

// Faces all of whose corner nodes are in the set (node_p[i] is the value of node i, in_set[i] != 0), fewer than three
// distinct nodes left out, faces whose node set occurs twice (interior faces) dropped, ascending by elem * 6 + face.
void PressureFaces(int64_t n_elem, const int32_t *conn, const std::vector<uint8_t> &in_set, const std::vector<double> &node_p,
                   std::vector<int32_t> *face_elem, std::vector<uint8_t> *face_id, std::vector<double> *face_p) {
    std::vector<Candidate> cand;
    for (int64_t e = 0; e < n_elem; e++)
        for (int f = 0; f < 6; f++) {
            const int32_t *nl = conn + 8 * e;
            int32_t nd[4];
            bool all = true;
            for (int k = 0; k < 4 && all; k++) { nd[k] = nl[FACE_NODES[f][k]]; all = in_set[(size_t)nd[k]] != 0; }
            if (!all) continue;
            Candidate c;
            c.elem = (int32_t)e; c.face = (uint8_t)f;
            c.p = 0.25 * (((node_p[(size_t)nd[0]] + node_p[(size_t)nd[1]]) + node_p[(size_t)nd[2]]) + node_p[(size_t)nd[3]]);
            std::sort(nd, nd + 4);
            const int distinct = (int)(std::unique(nd, nd + 4) - nd);
            if (distinct < 3) continue;
            for (int k = 0; k < 4; k++) c.key[(size_t)k] = k < distinct ? nd[k] : -1;
            cand.push_back(c);
        }
    std::sort(cand.begin(), cand.end(), [](const Candidate &a, const Candidate &b) {
        return a.key != b.key ? a.key < b.key : (a.elem != b.elem ? a.elem < b.elem : a.face < b.face);
    });
    std::vector<Candidate> keep;
    for (size_t i = 0; i < cand.size();) {
        size_t j = i + 1;
        while (j < cand.size() && cand[j].key == cand[i].key) j++;
        if (j - i == 1) keep.push_back(cand[i]);
        i = j;
    }
    std::sort(keep.begin(), keep.end(), [](const Candidate &a, const Candidate &b) {
        return a.elem != b.elem ? a.elem < b.elem : a.face < b.face;
    });
    face_elem->clear(); face_id->clear(); face_p->clear();
    for (const Candidate &c : keep) { face_elem->push_back(c.elem); face_id->push_back(c.face); face_p->push_back(c.p); }
}

bool HasDistributedLoads(const Database &db) {
    for (const auto &kv : db.BCLib.Items())
        if (kv.second.Type == "Pressure" || kv.second.Type == "BodyForce" || kv.second.Type == "Displacement") return true;
    return false;
}

int BuildDistributedLoads(const Database &db, const FlatModel &flat, const std::vector<int32_t> &red, DistributedLoads *out,
                          std::string *err) {
    auto fail = [&](const std::string &why) { if (err) *err = why; return STAN_HOST_E_ARG; };
    *out = DistributedLoads();
    const size_t nn = db.NodeLib.Count(), ne = flat.elem_mat.size(), nm = flat.mat_E_nu.size() / 2;
    if (flat.xyz.size() != nn * 3 || flat.conn.size() != ne * 8) return fail("the flat model does not belong to this database");
    // the elastic materials in MatLib order are the rows of mat_E_nu (Flatten)
    std::vector<std::pair<int, int>> mat_row;
    for (const auto &kv : db.MatLib.Items())
        if (kv.second.Type.find("Elastic") != std::string::npos) mat_row.emplace_back(kv.first, (int)mat_row.size());
    if (mat_row.size() != nm) return fail("the flat model does not belong to this database");
    for (const auto &kv : db.BCLib.Items()) {
        const BoundaryCondition &bc = kv.second;
        const bool pressure = bc.Type == "Pressure", body = bc.Type == "BodyForce", disp = bc.Type == "Displacement";
        if (!pressure && !body && !disp) continue;
        out->any = true;
        for (const auto &nv : bc.NodalValues.Items())
            if (nv.second.M.size() < 3) return fail(bc.Type + " value is not 3x1");
        if (body) {
            if (out->mat_body.empty()) out->mat_body.assign(nm * 3, 0.0);
            for (const auto &nv : bc.NodalValues.Items()) {   // keys are material IDs; several such BCs add up
                int row = -1;
                for (const auto &mr : mat_row) if (mr.first == nv.first) row = mr.second;
                if (row < 0) return fail("BodyForce on unknown (or not elastic) material " + std::to_string(nv.first));
                for (int d = 0; d < 3; d++) out->mat_body[(size_t)(3 * row + d)] += nv.second.M[(size_t)d];
            }
        } else if (pressure) {
            std::vector<uint8_t> in_set(nn, 0);
            std::vector<double> node_p(nn, 0.0);
            for (const auto &nv : bc.NodalValues.Items()) {
                const int64_t i = db.NodeLib.IndexOf(nv.first);
                if (i < 0) return fail("Pressure on unknown node " + std::to_string(nv.first));
                in_set[(size_t)i] = 1; node_p[(size_t)i] = nv.second.M[0];
            }
            std::vector<int32_t> fe; std::vector<uint8_t> fi; std::vector<double> fp;
            PressureFaces((int64_t)ne, flat.conn.data(), in_set, node_p, &fe, &fi, &fp);
            // merge into the canonical list: a face two BCs name carries the sum
            std::vector<int32_t> me; std::vector<uint8_t> mi; std::vector<double> mp;
            size_t a = 0, b = 0;
            auto key = [](int32_t e, uint8_t f) { return (int64_t)e * 6 + f; };
            while (a < out->face_elem.size() || b < fe.size()) {
                const int64_t ka = a < out->face_elem.size() ? key(out->face_elem[a], out->face_id[a]) : INT64_MAX;
                const int64_t kb = b < fe.size() ? key(fe[b], fi[b]) : INT64_MAX;
                if (ka < kb) { me.push_back(out->face_elem[a]); mi.push_back(out->face_id[a]); mp.push_back(out->face_p[a]); a++; }
                else if (kb < ka) { me.push_back(fe[b]); mi.push_back(fi[b]); mp.push_back(fp[b]); b++; }
                else { me.push_back(fe[b]); mi.push_back(fi[b]); mp.push_back(out->face_p[a] + fp[b]); a++; b++; }
            }
            out->face_elem.swap(me); out->face_id.swap(mi); out->face_p.swap(mp);
        } else {
            if (out->disp0.empty()) out->disp0.assign(nn * 3, 0.0);
            for (const auto &nv : bc.NodalValues.Items()) {
                const int64_t i = db.NodeLib.IndexOf(nv.first);
                if (i < 0) return fail("Displacement on unknown node " + std::to_string(nv.first));
                for (int d = 0; d < 3; d++) {
                    const int32_t dof = flat.node_dof[(size_t)(3 * i + d)];
                    if (dof < 0 || (size_t)dof >= red.size()) return fail("DOF outside nDOF");
                    const double v = nv.second.M[(size_t)d];
                    if (red[(size_t)dof] == -1) {
                        out->disp0[(size_t)(3 * i + d)] = v;
                    } else if (v != 0.0) {
                        return fail("Displacement on node " + std::to_string(nv.first) + ", direction " + "XYZ"[d] +
                                    ": the DOF is free (an SPC must fix it)");
                    }   // a zero component on a free DOF is ignored
                }
            }
        }
    }
    for (double v : out->disp0) out->n_prescribed += v != 0.0;
    return STAN_HOST_OK;
}

bool HasThermalLoads(const Database &db) {
    for (const auto &kv : db.BCLib.Items())
        if (kv.second.Type == "Temperature" || kv.second.Type == "ThermalExpansion") return true;
    return false;
}

int BuildThermalLoads(const Database &db, const FlatModel &flat, ThermalLoads *out, std::string *err) {
    auto fail = [&](const std::string &why) { if (err) *err = why; return STAN_HOST_E_ARG; };
    *out = ThermalLoads();
    const size_t nn = db.NodeLib.Count(), nm = flat.mat_E_nu.size() / 2;
    if (flat.xyz.size() != nn * 3) return fail("the flat model does not belong to this database");
    // the elastic materials in MatLib order are the rows of mat_E_nu (Flatten)
    std::vector<std::pair<int, int>> mat_row;
    for (const auto &kv : db.MatLib.Items())
        if (kv.second.Type.find("Elastic") != std::string::npos) mat_row.emplace_back(kv.first, (int)mat_row.size());
    if (mat_row.size() != nm) return fail("the flat model does not belong to this database");
    out->mat_alpha.assign(nm, 0.0);
    out->dT.assign(nn, 0.0);
    for (const auto &kv : db.BCLib.Items()) {
        const BoundaryCondition &bc = kv.second;
        const bool temp = bc.Type == "Temperature", expansion = bc.Type == "ThermalExpansion";
        if (!temp && !expansion) continue;
        out->any = true;
        for (const auto &nv : bc.NodalValues.Items()) {   // several such BCs add up
            if (nv.second.M.size() < 3) return fail(bc.Type + " value is not 3x1");
            if (temp) {
                const int64_t i = db.NodeLib.IndexOf(nv.first);
                if (i < 0) return fail("Temperature on unknown node " + std::to_string(nv.first));
                out->dT[(size_t)i] += nv.second.M[0];
            } else {                                      // keys are material IDs
                int row = -1;
                for (const auto &mr : mat_row) if (mr.first == nv.first) row = mr.second;
                if (row < 0) return fail("ThermalExpansion on unknown (or not elastic) material " + std::to_string(nv.first));
                out->mat_alpha[(size_t)row] += nv.second.M[0];
            }
        }
    }
    return STAN_HOST_OK;
}

bool HasDensity(const Database &db) {
    for (const auto &kv : db.BCLib.Items())
        if (kv.second.Type == "Density") return true;
    return false;
}

int BuildDensity(const Database &db, const FlatModel &flat, MassDensity *out, std::string *err) {
    auto fail = [&](const std::string &why) { if (err) *err = why; return STAN_HOST_E_ARG; };
    *out = MassDensity();
    const size_t nm = flat.mat_E_nu.size() / 2;
    // the elastic materials in MatLib order are the rows of mat_E_nu (Flatten)
    std::vector<std::pair<int, int>> mat_row;
    for (const auto &kv : db.MatLib.Items())
        if (kv.second.Type.find("Elastic") != std::string::npos) mat_row.emplace_back(kv.first, (int)mat_row.size());
    if (mat_row.size() != nm) return fail("the flat model does not belong to this database");
    out->mat_rho.assign(nm, 0.0);
    for (const auto &kv : db.BCLib.Items()) {
        const BoundaryCondition &bc = kv.second;
        if (bc.Type != "Density") continue;
        out->any = true;
        for (const auto &nv : bc.NodalValues.Items()) {   // keys are material IDs; several such BCs add up
            if (nv.second.M.size() < 3) return fail("Density value is not 3x1");
            int row = -1;
            for (const auto &mr : mat_row) if (mr.first == nv.first) row = mr.second;
            if (row < 0) return fail("Density on unknown (or not elastic) material " + std::to_string(nv.first));
            out->mat_rho[(size_t)row] += nv.second.M[0];
        }
    }
    return STAN_HOST_OK;
}

}  // namespace stan

extern "C" {

int stan_host_pressure_faces(int64_t n_nodes, int64_t n_elem, const int32_t *conn, int64_t n_set, const int32_t *set_nodes,
                             const double *set_p, int64_t capacity, int32_t *face_elem, uint8_t *face_id, double *face_p,
                             int64_t *n_faces) {
    if (n_nodes <= 0 || n_elem < 0 || n_set < 0 || !n_faces || (n_elem > 0 && !conn) || (n_set > 0 && (!set_nodes || !set_p)))
        return STAN_HOST_E_ARG;
    for (int64_t t = 0; t < n_elem * 8; t++)
        if (conn[t] < 0 || conn[t] >= n_nodes) return STAN_HOST_E_ARG;
    std::vector<uint8_t> in_set((size_t)n_nodes, 0);
    std::vector<double> node_p((size_t)n_nodes, 0.0);
    for (int64_t k = 0; k < n_set; k++) {
        if (set_nodes[k] < 0 || set_nodes[k] >= n_nodes) return STAN_HOST_E_ARG;
        in_set[(size_t)set_nodes[k]] = 1; node_p[(size_t)set_nodes[k]] = set_p[k];
    }
    std::vector<int32_t> fe; std::vector<uint8_t> fi; std::vector<double> fp;
    stan::PressureFaces(n_elem, conn, in_set, node_p, &fe, &fi, &fp);
    *n_faces = (int64_t)fe.size();
    if (!face_elem && !face_id && !face_p) return STAN_HOST_OK;   // sizing call
    if (!face_elem || !face_id || !face_p || capacity < *n_faces) return STAN_HOST_E_ARG;
    std::copy(fe.begin(), fe.end(), face_elem);
    std::copy(fi.begin(), fi.end(), face_id);
    std::copy(fp.begin(), fp.end(), face_p);
    return STAN_HOST_OK;
}

}  // extern "C"
