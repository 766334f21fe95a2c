// vtu.cpp -- VTK XML UnstructuredGrid writer: what Part.ExportGrid + ExportWindow.Export_Click leave on disk
// (Part.cs:858-939, ExportWindow.xaml.cs:43-108), without VTK.  One piece over the whole model in wire order; points are
// the deformed coordinates xyz + disp (Part.UpdateNode, Part.cs:581-594) as Float64; a cell is the element's 8 nodes in
// CHEXA order = VTK_HEXAHEDRON's (Part.cs:879-885); every scalar array is Float32 (the reference holds vtkFloatArray).
// All arrays sit in ONE <AppendedData encoding="raw"> block, uncompressed, each prefixed with its byte count as UInt64.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/stan_host.h"

namespace {

// Part.cs:403-428 (point arrays; the cell arrays of :272-297 carry a "Max " / "Average " / "Min " prefix)
const char *const SCALAR_NAMES[24] = {
    "Displacement X", "Displacement Y", "Displacement Z", "Total Displacement",
    "Stress XX", "Stress YY", "Stress ZZ", "Stress XY", "Stress YZ", "Stress XZ",
    "Stress P1", "Stress P2", "Stress P3", "von Mises Stress",
    "Strain XX", "Strain YY", "Strain ZZ", "Strain XY", "Strain YZ", "Strain XZ",
    "Strain P1", "Strain P2", "Strain P3", "Effective Strain"};

std::string xml_escape(const char *s) {
    std::string o;
    for (; *s; s++) {
        if (*s == '&') o += "&amp;";
        else if (*s == '<') o += "&lt;";
        else if (*s == '>') o += "&gt;";
        else if (*s == '"') o += "&quot;";
        else o += *s;
    }
    return o;
}

struct appended {   // offsets of the arrays inside the appended block, in the order they will be written
    uint64_t at = 0;
    uint64_t add(uint64_t bytes) { const uint64_t o = at; at += 8 + bytes; return o; }
};

bool put(FILE *f, const void *p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }
bool put_size(FILE *f, uint64_t bytes) { return put(f, &bytes, 8); }

// n values produced by fn(i), written through a bounded buffer
template <typename T, typename F>
bool put_array(FILE *f, uint64_t n, F fn) {
    if (!put_size(f, n * sizeof(T))) return false;
    std::vector<T> buf((size_t)(n < 65536 ? n : 65536));
    for (uint64_t i0 = 0; i0 < n; i0 += 65536) {
        const uint64_t m = n - i0 < 65536 ? n - i0 : 65536;
        for (uint64_t i = 0; i < m; i++) buf[(size_t)i] = fn(i0 + i);
        if (!put(f, buf.data(), (size_t)m * sizeof(T))) return false;
    }
    return true;
}

}  // namespace

extern "C" {

const char *stan_host_scalar_name(int32_t s) { return s >= 0 && s < 24 ? SCALAR_NAMES[s] : nullptr; }

int stan_host_write_vtu(const char *path, int64_t n_nodes, const double *xyz, const double *disp, int64_t n_elem,
                        const int32_t *conn, int32_t n_point_arrays, const char *const *names, const double *point_values,
                        int32_t n_cell_arrays, const char *const *cell_names, const double *cell_values) {
    return stan_host_write_vtu_components(path, n_nodes, xyz, disp, n_elem, conn, n_point_arrays, names, nullptr, point_values, n_cell_arrays,
                                          cell_names, cell_values);
}

int stan_host_write_vtu_components(const char *path, int64_t n_nodes, const double *xyz, const double *disp, int64_t n_elem,
                                   const int32_t *conn, int32_t n_point_arrays, const char *const *names, const int32_t *point_components,
                                   const double *point_values, int32_t n_cell_arrays, const char *const *cell_names,
                                   const double *cell_values) {
    auto comps = [&](int32_t k) { return point_components ? point_components[k] : 1; };
    for (int32_t k = 0; point_components && k < n_point_arrays; k++)
        if (point_components[k] < 1) return STAN_HOST_E_ARG;
    if (!path || n_nodes <= 0 || !xyz || n_elem < 0 || (n_elem > 0 && !conn) || n_point_arrays < 0 || n_cell_arrays < 0 ||
        (n_point_arrays > 0 && (!names || !point_values)) || (n_cell_arrays > 0 && (!cell_names || !cell_values)))
        return STAN_HOST_E_ARG;
    for (int64_t t = 0; t < n_elem * 8; t++)
        if (conn[t] < 0 || conn[t] >= n_nodes) return STAN_HOST_E_ARG;
    for (int32_t k = 0; k < n_point_arrays; k++) if (!names[k]) return STAN_HOST_E_ARG;
    for (int32_t k = 0; k < n_cell_arrays; k++) if (!cell_names[k]) return STAN_HOST_E_ARG;
    const uint64_t nn = (uint64_t)n_nodes, ne = (uint64_t)n_elem;
    appended ap;
    std::string head = "<?xml version=\"1.0\"?>\n<VTKFile type=\"UnstructuredGrid\" version=\"1.0\" byte_order=\"LittleEndian\" "
                       "header_type=\"UInt64\">\n  <UnstructuredGrid>\n    <Piece NumberOfPoints=\"" + std::to_string(nn) +
                       "\" NumberOfCells=\"" + std::to_string(ne) + "\">\n";
    auto array = [&](const char *type, const std::string &name, int ncomp, uint64_t bytes) {
        head += "        <DataArray type=\"" + std::string(type) + "\"" + (name.empty() ? "" : " Name=\"" + name + "\"") +
                (ncomp > 1 ? " NumberOfComponents=\"" + std::to_string(ncomp) + "\"" : "") +
                " format=\"appended\" offset=\"" + std::to_string(ap.add(bytes)) + "\"/>\n";
    };
    head += "      <Points>\n";
    array("Float64", "Points", 3, nn * 24);
    head += "      </Points>\n      <Cells>\n";
    array("Int64", "connectivity", 1, ne * 64);
    array("Int64", "offsets", 1, ne * 8);
    array("UInt8", "types", 1, ne);
    head += "      </Cells>\n      <PointData>\n";
    for (int32_t k = 0; k < n_point_arrays; k++) array("Float32", xml_escape(names[k]), comps(k), nn * 4 * (uint64_t)comps(k));
    head += "      </PointData>\n      <CellData>\n";
    for (int32_t k = 0; k < n_cell_arrays; k++) array("Float32", xml_escape(cell_names[k]), 1, ne * 4);
    head += "      </CellData>\n    </Piece>\n  </UnstructuredGrid>\n  <AppendedData encoding=\"raw\">\n   _";

    FILE *f = fopen(path, "wb");
    if (!f) return STAN_HOST_E_IO;
    std::vector<char> iobuf((size_t)1 << 20);
    setvbuf(f, iobuf.data(), _IOFBF, iobuf.size());
    bool ok = put(f, head.data(), head.size());
    ok = ok && put_array<double>(f, nn * 3, [&](uint64_t i) { return disp ? xyz[i] + disp[i] : xyz[i]; });
    ok = ok && put_array<int64_t>(f, ne * 8, [&](uint64_t i) { return (int64_t)conn[i]; });
    ok = ok && put_array<int64_t>(f, ne, [&](uint64_t i) { return (int64_t)(8 * (i + 1)); });
    ok = ok && put_array<uint8_t>(f, ne, [&](uint64_t) { return (uint8_t)12; });   // VTK_HEXAHEDRON
    const double *pv = point_values;   // array k: [n_nodes][comps(k)]
    for (int32_t k = 0; ok && k < n_point_arrays; k++) {
        const uint64_t n = nn * (uint64_t)comps(k);
        ok = put_array<float>(f, n, [&](uint64_t i) { return (float)pv[i]; });
        pv += n;
    }
    for (int32_t k = 0; ok && k < n_cell_arrays; k++) {
        const double *v = cell_values + (uint64_t)k * ne;
        ok = put_array<float>(f, ne, [&](uint64_t i) { return (float)v[i]; });
    }
    static const char tail[] = "\n  </AppendedData>\n</VTKFile>\n";
    ok = ok && put(f, tail, sizeof(tail) - 1);
    ok = (fclose(f) == 0) && ok;
    return ok ? STAN_HOST_OK : STAN_HOST_E_IO;
}

}  // extern "C"
