// Stand-alone host program over include/rdc_marshal.h (no device, no library: it links tests/fake_rdc_handback.cpp), driven by
// tests/test_host_marshal.py and, without arguments, by tools/asan_marshal.sh:
//   tables                                   every key table as "<struct> <key> <offset> <real|int>"
//   read <mirror|minimal> <struct> <in> <out>  the struct read from a case file through that kind of store, as raw bytes
//   solid <mirror|minimal> <in>              solid parameters, material table and side list of a case file
//   handback <n_nodes> <n_chunks>            the pipelined hand-back against the fake, every call logged
// The header is instantiated with two parameter stores: the host mirror's Parameters and MinimalStore below, which has
// get / have_parameter and nothing else, and a point type of its own -- what the header may ask of libMesh::Parameters.
// Case files: "<key> <value>" is a real (an int for RT_dose/total/max); "string|bool|point <key> <value...>",
// "subdomains <id...>" and "side <elem> <side> <id>" give the rest of a solid case.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../include/rdc_marshal.h"
#include "../rdcfes_amd/host/rdc_host.h"

using namespace rdc;

extern "C" {
rdc_ctx* fake_ctx_new(int nvar, const int64_t* row_ptr, const double* val, const double* rhs);
void fake_ctx_delete(rdc_ctx* c);
void fake_fail(rdc_ctx* c, const char* call);
}

struct Vec3 {
  double c[3];
  double operator()(int d) const { return c[d]; }
};

class MinimalStore {
 public:
  template <class T> const T& get(const std::string& key) const {
    auto it = map<T>().find(key);
    if (it == map<T>().end()) throw std::runtime_error("MinimalStore: no parameter '" + key + "'");
    return it->second;
  }
  template <class T> bool have_parameter(const std::string& key) const { return map<T>().count(key) != 0; }
  template <class T> std::map<std::string, T>& map() const {
    if constexpr (std::is_same_v<T, double>) return r_;
    else if constexpr (std::is_same_v<T, int>) return i_;
    else if constexpr (std::is_same_v<T, bool>) return b_;
    else if constexpr (std::is_same_v<T, std::string>) return s_;
    else return p_;
  }
 private:
  mutable std::map<std::string, double> r_;
  mutable std::map<std::string, int> i_;
  mutable std::map<std::string, bool> b_;
  mutable std::map<std::string, std::string> s_;
  mutable std::map<std::string, Vec3> p_;
};

template <class T> void put(host::Parameters& P, const std::string& k, const T& v) { P.set<T>(k) = v; }
template <class T> void put(MinimalStore& P, const std::string& k, const T& v) { P.map<T>()[k] = v; }
inline host::Point point(const host::Parameters&, double x, double y, double z) { return host::Point(x, y, z); }
inline Vec3 point(const MinimalStore&, double x, double y, double z) { return Vec3{{x, y, z}}; }
template <class P> struct PointOf { using type = host::Point; };
template <> struct PointOf<MinimalStore> { using type = Vec3; };

struct Case {
  std::vector<int> subdomain;
  struct Side { int64_t elem; int32_t side; int id; };
  std::vector<Side> sides;
  double time = 0.0;
};

template <class P> Case load(const std::string& file, P& params) {
  std::ifstream in(file);
  if (!in) throw std::runtime_error("cannot open " + file);
  Case c;
  std::string line, w, key;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    if (!(ls >> w)) continue;
    if (w == "string") { ls >> key; std::string rest; std::getline(ls >> std::ws, rest); put(params, key, rest); }
    else if (w == "bool") { int b; ls >> key >> b; put(params, key, b != 0); }
    else if (w == "point") {   // strtod: a component may be "nan" (not constrained)
      std::string x, y, z;
      ls >> key >> x >> y >> z;
      put(params, key, point(params, std::strtod(x.c_str(), nullptr), std::strtod(y.c_str(), nullptr), std::strtod(z.c_str(), nullptr)));
    }
    else if (w == "subdomains") { int id; while (ls >> id) c.subdomain.push_back(id); }
    else if (w == "side") { Case::Side s; ls >> s.elem >> s.side >> s.id; c.sides.push_back(s); }
    else {
      std::string v;
      ls >> v;
      if (w == "RT_dose/total/max") put(params, w, std::atoi(v.c_str()));
      else put(params, w, std::atof(v.c_str()));
      if (w == "time") c.time = std::atof(v.c_str());
    }
  }
  return c;
}

template <class S> void dump_table(const char* name) {
  for (const marshal::Key& k : marshal::keys<S>()) std::printf("%s %s %zu %s\n", name, k.key.c_str(), k.offset, k.is_int ? "int" : "real");
}

template <class S> std::string bytes_of(const S& s) { return std::string(reinterpret_cast<const char*>(&s), sizeof s); }

template <class P> std::string read_struct(const std::string& name, const P& params, double time) {
  if (name == "pihna") return bytes_of(marshal::read<rdc_pihna_params>(params));
  if (name == "ripf") return bytes_of(marshal::read<rdc_ripf_params>(params));
  if (name == "hcc") return bytes_of(marshal::read<rdc_hcc_params>(params));
  if (name == "adpm") return bytes_of(marshal::read_adpm(params, time));
  if (name == "proteas") return bytes_of(marshal::read<rdc_proteas_params>(params));
  if (name == "pihna_ranges") return bytes_of(marshal::read<rdc_pihna_ranges>(params));
  if (name == "ripf_ranges") return bytes_of(marshal::read<rdc_ripf_ranges>(params));
  throw std::runtime_error("unknown struct " + name);
}

template <class P> void mode_read(const std::string& name, const std::string& in, const std::string& out) {
  P params;
  const Case c = load(in, params);
  const std::string b = read_struct(name, params, c.time);
  std::ofstream(out, std::ios::binary).write(b.data(), (std::streamsize)b.size());
}

template <class P> void mode_solid(const std::string& in) {
  P params;
  const Case c = load(in, params);
  const rdc_solid_params sp = marshal::solid_params(params);
  std::printf("params %.17g %.17g %d %d\n", sp.pseudo_time, sp.displacement_penalty, sp.use_symmetry, sp._pad);
  const marshal::MaterialTable mt = marshal::material_table(params, (int64_t)c.subdomain.size(), [&](int64_t e) { return c.subdomain[(size_t)e]; });
  std::printf("elem_material");
  for (int32_t m : mt.elem_material) std::printf(" %d", m);
  std::printf("\n");
  for (const rdc_solid_material& m : mt.table)
    std::printf("material %.17g %.17g %.17g %.17g %.17g %.17g\n", m.Young, m.Poisson, m.FibreStiffness, m.rate[0], m.rate[1], m.rate[2]);
  const marshal::SideList sl = marshal::side_list<typename PointOf<P>::type>(params, [&](int bc, auto&& emit) {
    for (const Case::Side& s : c.sides) if (s.id == bc) emit(s.elem, s.side);
  });
  for (size_t i = 0; i < sl.elem.size(); i++)
    std::printf("side %lld %d %.17g %.17g %.17g\n", (long long)sl.elem[i], sl.side[i], sl.displacement[3 * i], sl.displacement[3 * i + 1], sl.displacement[3 * i + 2]);
}

// nvar = 2; the rows of node n hold 1 + n % 3 values each.  "# ..." lines say what the program does between the fake's lines.
static void mode_handback(int64_t n_nodes, int n_chunks) {
  const int nvar = 2;
  std::vector<int64_t> row_ptr(1, 0);
  for (int64_t r = 0; r < n_nodes * nvar; r++) row_ptr.push_back(row_ptr.back() + 1 + (r / nvar) % 3);
  std::vector<double> src_val((size_t)row_ptr.back()), src_rhs((size_t)(n_nodes * nvar));
  std::vector<double> val(src_val.size()), rhs(src_rhs.size());
  rdc_ctx* c = fake_ctx_new(nvar, row_ptr.data(), src_val.data(), src_rhs.data());
  marshal::PinState pins;
  int pass = 0;
  auto hand_back = [&] {
    pass++;
    for (size_t i = 0; i < src_val.size(); i++) src_val[i] = 1000.0 * pass + (double)i;
    for (size_t i = 0; i < src_rhs.size(); i++) src_rhs[i] = -1000.0 * pass - (double)i;
    std::fill(val.begin(), val.end(), 0.0);
    std::fill(rhs.begin(), rhs.end(), 0.0);
    std::printf("# handback %d val %p rhs %p\n", pass, (void*)val.data(), (void*)rhs.data());
    marshal::hand_back_chunked(c, n_nodes, n_chunks, val.data(), val.size(), rhs.data(), rhs.size(), pins, [&](int64_t n0, int64_t n1) {
      bool ok = true;   // the rows of the chunk are there when it is consumed
      for (int64_t k = row_ptr[(size_t)(n0 * nvar)]; k < row_ptr[(size_t)(n1 * nvar)]; k++) ok &= val[(size_t)k] == src_val[(size_t)k];
      for (int64_t r = n0 * nvar; r < n1 * nvar; r++) ok &= rhs[(size_t)r] == src_rhs[(size_t)r];
      std::printf("consume %lld %lld %s\n", (long long)n0, (long long)n1, ok ? "ok" : "BAD");
    });
    std::printf("# equal %d\n", (int)(val == src_val && rhs == src_rhs));
  };
  hand_back();
  hand_back();
  std::printf("# release\n");
  marshal::check(c, pins.release(c), "rdc_host_unpin");
  hand_back();
  std::vector<double> moved(val.size());   // val "reallocates": other storage of the same size
  val.swap(moved);
  std::printf("# reallocated\n");
  hand_back();
  fake_fail(c, "rdc_ticket_wait");
  try {
    hand_back();
    std::printf("# error none\n");
  } catch (const std::runtime_error& e) {
    std::printf("# error %s\n", e.what());
  }
  std::printf("# release\n");
  marshal::check(c, pins.release(c), "rdc_host_unpin");
  fake_ctx_delete(c);
}

// no arguments: every routine once on inputs made from the key tables themselves (the sanitizer run)
template <class S, class P> void self_read(P& params) {
  double x = 1.0;
  for (const marshal::Key& k : marshal::keys<S>()) { if (k.is_int) put(params, k.key, 7); else put(params, k.key, x); x += 1.0; }
  const S s = marshal::read<S>(params);
  x = 1.0;
  for (const marshal::Key& k : marshal::keys<S>()) {
    if (k.offset + (k.is_int ? sizeof(int32_t) : sizeof(double)) > sizeof(S)) throw std::runtime_error("offset outside the struct: " + k.key);
    double v = 0.0;
    if (!k.is_int) std::memcpy(&v, reinterpret_cast<const char*>(&s) + k.offset, sizeof v);
    if (!k.is_int && v != x) throw std::runtime_error("field of " + k.key + " holds another value");
    x += 1.0;
  }
}
template <class P> void self_check() {
  { P p; self_read<rdc_pihna_params>(p); }
  { P p; self_read<rdc_ripf_params>(p); }
  { P p; self_read<rdc_hcc_params>(p); }
  { P p; self_read<rdc_adpm_params>(p); }
  { P p; self_read<rdc_proteas_params>(p); }
  { P p; self_read<rdc_pihna_ranges>(p); }
  { P p; self_read<rdc_ripf_ranges>(p); }
  P p;
  put(p, "pseudo_time", 0.5); put(p, "BCs/displacement_penalty", 1e5); put(p, "solver/assembly_use_symmetry", true);
  put(p, "BCs", std::string("2 5"));
  for (int bc : {2, 5}) put(p, "BC/" + std::to_string(bc) + "/displacement", point(p, 1.0 * bc, 0.0, -1.0));
  for (int id : {3, 7, 9})
    for (const char* f : {"Young", "Poisson", "FibreStiffness", "VolumetricStretchRatio/rate_0", "VolumetricStretchRatio/rate_1", "VolumetricStretchRatio/rate_2"})
      put(p, "material/" + std::to_string(id) + "/Hyperelastic/" + f, 1.0 * id);
  const int sub[6] = {7, 3, 7, 9, 3, 3};
  const marshal::MaterialTable mt = marshal::material_table(p, 6, [&](int64_t e) { return sub[e]; });
  const marshal::SideList sl = marshal::side_list<typename PointOf<P>::type>(p, [&](int bc, auto&& emit) { emit(bc, 1); });
  if (mt.table.size() != 3 || sl.elem.size() != 2 || marshal::solid_params(p).use_symmetry != 1) throw std::runtime_error("solid pieces");
}

int main(int argc, char** argv) {
  try {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "tables") {
      dump_table<rdc_pihna_params>("pihna"); dump_table<rdc_ripf_params>("ripf"); dump_table<rdc_hcc_params>("hcc");
      dump_table<rdc_adpm_params>("adpm"); dump_table<rdc_proteas_params>("proteas");
      dump_table<rdc_pihna_ranges>("pihna_ranges"); dump_table<rdc_ripf_ranges>("ripf_ranges");
    } else if (mode == "read" && argc == 6) {
      if (std::string(argv[2]) == "minimal") mode_read<MinimalStore>(argv[3], argv[4], argv[5]);
      else mode_read<host::Parameters>(argv[3], argv[4], argv[5]);
    } else if (mode == "solid" && argc == 4) {
      if (std::string(argv[2]) == "minimal") mode_solid<MinimalStore>(argv[3]);
      else mode_solid<host::Parameters>(argv[3]);
    } else if (mode == "handback" && argc == 4) {
      mode_handback(std::atoll(argv[2]), std::atoi(argv[3]));
    } else if (argc == 1) {
      self_check<host::Parameters>();
      self_check<MinimalStore>();
      const int cases[4][2] = {{27, 1}, {27, 2}, {27, 7}, {5, 40}};
      for (auto& nc : cases) mode_handback(nc[0], nc[1]);
    } else {
      std::fprintf(stderr, "usage: host_marshal_main [tables | read <store> <struct> <in> <out> | solid <store> <in> | handback <n_nodes> <n_chunks>]\n");
      return 2;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "host_marshal_main failed: %s\n", e.what());
    return 1;
  }
  return 0;
}
