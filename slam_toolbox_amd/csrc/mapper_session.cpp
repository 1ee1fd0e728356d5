// Mapping sessions of the mapper front end: save, load, resume (slam_toolbox's serializePoseGraph / deserializePoseGraph +
// loadSerializedPoseGraph, slam_toolbox_common.cpp:952-1017).
// The file is the library's own format (DESIGN.md section 7 has it byte by byte):
//   header   "KHMS", u32 version, u64 file size, u32 section count, u32 CRC-32 (IEEE, as zlib's) of everything behind the header
//   table    per section: 4-byte tag, u32 0, u64 offset, u64 size; the sections follow in table order, each a multiple of 8 bytes
//   PARM LASR LIFE STAT RUNB SCAN RNGS ADJL SNOD SCON SANA
// All integers and doubles little endian.  Parsing never trusts a count: every section's size is recomputed from the counts of
// STAT / its own head in 128-bit arithmetic and compared with the table before anything is read through it.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "mapper_private.hpp"
#include "spa_internal.hpp"

namespace kh
{
namespace mapper
{
namespace
{
static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the session file is written by memcpy: little-endian hosts only");
constexpr uint32_t kSessionVersion = 1;
constexpr int kSections = 11;
const char kSectionTags[kSections][5] = {"PARM", "LASR", "LIFE", "STAT", "RUNB", "SCAN", "RNGS", "ADJL", "SNOD", "SCON", "SANA"};
constexpr size_t kHeaderBytes = 24, kTableBytes = 24 * kSections;
double g_last_load_ms[4] = {0.0, 0.0, 0.0, 0.0};      // kh_session_last_load_ms

uint32_t crc32_ieee(const uint8_t * p, size_t n)
{
  static const std::vector<uint32_t> table = [] {
      std::vector<uint32_t> t(256);
      for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) {c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;}
        t[i] = c;
      }
      return t;
    }();
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);}
  return c ^ 0xFFFFFFFFu;
}

// kh_mapper_params as 29 words of 8 bytes in declaration order: the int32 fields as int64, the doubles as they are
#define KH_SESSION_PARAM_WORDS(I, D)                                                                                              \
  I(use_scan_matching) I(use_scan_barycenter) D(minimum_time_interval) D(minimum_travel_distance) D(minimum_travel_heading)      \
  I(scan_buffer_size) D(scan_buffer_maximum_scan_distance) D(link_match_minimum_response_fine) D(link_scan_maximum_distance)     \
  D(loop_search_maximum_distance) I(do_loop_closing) I(loop_match_minimum_chain_size) D(loop_match_maximum_variance_coarse)      \
  D(loop_match_minimum_response_coarse) D(loop_match_minimum_response_fine) D(correlation_search_space_dimension)                \
  D(correlation_search_space_resolution) D(correlation_search_space_smear_deviation) D(loop_search_space_dimension)              \
  D(loop_search_space_resolution) D(loop_search_space_smear_deviation) D(match.coarse_search_angle_offset)                       \
  D(match.coarse_angle_resolution) D(match.fine_search_angle_offset) I(match.use_response_expansion)                             \
  D(match.distance_variance_penalty) D(match.minimum_distance_penalty) D(match.angle_variance_penalty) D(match.minimum_angle_penalty)
constexpr size_t kParamWords = 29, kLaserWords = 9, kLifeWords = 9, kStatWords = 6;

struct Blob
{
  std::string b;
  void raw(const void * p, size_t n) {b.append(static_cast<const char *>(p), n);}
  void i64(int64_t v) {raw(&v, 8);}
  void f64(double v) {raw(&v, 8);}
  void i32s(const std::vector<int32_t> & v) {if (!v.empty()) {raw(v.data(), 4 * v.size());}}
  void pad8() {while (b.size() % 8) {b.push_back('\0');}}
};

// what a session file holds, as parsed (and as kh_mapper_load puts it into a mapper)
struct Session
{
  kh_mapper_params p; kh_laser laser; int64_t lifelong = 0; kh_decay_params decay;
  int64_t n_slots = 0, n_alive = 0, n_edges = 0, last = -1, n_running = 0, n_loc = 0;
  std::vector<int32_t> running, loc;
  std::vector<int32_t> ids; std::vector<double> time, odom, corr, score, ranges;
  std::vector<int32_t> adj_count, out_count, adj, out;
  int64_t n_nodes = 0, words[7] = {0, 0, 0, 0, 0, 0, 0};
  std::vector<int32_t> node_ids; std::vector<double> node_poses;
  int64_t n_cons = 0;
  std::vector<int32_t> ca, cb; std::vector<double> cz, cinfo;
  int64_t n_sn = 0;
  std::vector<int32_t> sn_ptr, sn_ids;
  int64_t version = 0, file_bytes = 0;
};

bool read_file(const char * path, std::string & out)
{
  FILE * f = std::fopen(path, "rb");
  if (!f) {return false;}
  char buf[1 << 16];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) {out.append(buf, n);}
  const bool ok = !std::ferror(f);
  std::fclose(f);
  return ok;
}

int bad_file(const std::string & why)
{
  set_error("session file: " + why);
  return KH_ERR_IO;
}

typedef unsigned __int128 u128;
inline uint64_t round8(uint64_t v) {return (v + 7) & ~static_cast<uint64_t>(7);}

// bounds-checked cursor over one section
struct Cursor
{
  const uint8_t * p; size_t left;
  bool take(void * dst, size_t n) {if (n > left) {return false;} if (n) {std::memcpy(dst, p, n);} p += n; left -= n; return true;}
  bool skip(size_t n) {if (n > left) {return false;} p += n; left -= n; return true;}
  template <class T> bool vec(std::vector<T> & v, uint64_t count)
  {
    if (static_cast<u128>(count) * sizeof(T) > left) {return false;}
    v.resize(static_cast<size_t>(count));
    return take(v.data(), static_cast<size_t>(count) * sizeof(T));
  }
};

// header, table, checksum, every section's size against its counts, and every id against the lists it indexes
int parse_session(const std::string & data, Session & S)
{
  const uint8_t * base = reinterpret_cast<const uint8_t *>(data.data());
  const uint64_t size = data.size();
  if (size < kHeaderBytes) {return bad_file("truncated inside the header");}
  if (std::memcmp(base, "KHMS", 4) != 0) {return bad_file("wrong magic (not a mapping session)");}
  uint32_t version, n_sections, crc; uint64_t file_size;
  std::memcpy(&version, base + 4, 4); std::memcpy(&file_size, base + 8, 8); std::memcpy(&n_sections, base + 16, 4); std::memcpy(&crc, base + 20, 4);
  if (version != kSessionVersion) {return bad_file("unknown version " + std::to_string(version));}
  if (file_size != size) {return bad_file("truncated: the header says " + std::to_string(file_size) + " bytes, the file has " + std::to_string(size));}
  if (n_sections != kSections || size < kHeaderBytes + kTableBytes) {return bad_file("section table does not fit");}
  if (crc32_ieee(base + kHeaderBytes, static_cast<size_t>(size - kHeaderBytes)) != crc) {return bad_file("checksum mismatch");}
  uint64_t off[kSections], len[kSections], at = kHeaderBytes + kTableBytes;
  for (int k = 0; k < kSections; ++k) {
    const uint8_t * e = base + kHeaderBytes + 24 * k;
    uint32_t zero;
    std::memcpy(&zero, e + 4, 4); std::memcpy(&off[k], e + 8, 8); std::memcpy(&len[k], e + 16, 8);
    if (std::memcmp(e, kSectionTags[k], 4) != 0 || zero != 0) {return bad_file("section table: unexpected tag");}
    if (off[k] != at || (len[k] & 7) || len[k] > size - at) {return bad_file(std::string("section ") + kSectionTags[k] + " does not fit the file");}
    at += len[k];
  }
  if (at != size) {return bad_file("bytes behind the last section");}
  S.version = version; S.file_bytes = static_cast<int64_t>(size);
  auto cursor = [&](int k) {return Cursor{base + off[k], static_cast<size_t>(len[k])};};
  auto misfit = [&](int k) {return bad_file(std::string("counts do not fit section ") + kSectionTags[k]);};
  // PARM, LASR, LIFE, STAT: fixed size
  if (len[0] != 8 * kParamWords || len[1] != 8 * kLaserWords || len[2] != 8 * kLifeWords || len[3] != 8 * kStatWords) {return misfit(0);}
  {
    Cursor c = cursor(0);
    int64_t iv;
#define KH_RD_I(f) c.take(&iv, 8); S.p.f = static_cast<int32_t>(iv);
#define KH_RD_D(f) c.take(&S.p.f, 8);
    KH_SESSION_PARAM_WORDS(KH_RD_I, KH_RD_D)
#undef KH_RD_I
#undef KH_RD_D
    c = cursor(1);
    c.take(&iv, 8);
    if (iv < 1 || iv > (1 << 20)) {return bad_file("laser: beam count out of range");}
    S.laser.n_beams = static_cast<int32_t>(iv);
    c.take(&S.laser.minimum_angle, 8); c.take(&S.laser.angular_resolution, 8); c.take(&S.laser.minimum_range, 8); c.take(&S.laser.maximum_range, 8);
    c.take(&S.laser.range_threshold, 8); c.take(&S.laser.offset_x, 8); c.take(&S.laser.offset_y, 8); c.take(&S.laser.offset_heading, 8);
    c = cursor(2);
    c.take(&S.lifelong, 8);
    c.take(&S.decay.iou_thresh, 8); c.take(&S.decay.iou_match, 8); c.take(&S.decay.removal_score, 8); c.take(&S.decay.overlap_scale, 8);
    c.take(&S.decay.constraint_scale, 8); c.take(&S.decay.nearby_penalty, 8); c.take(&S.decay.candidates_scale, 8);
    c.take(&iv, 8); S.decay.scan_buffer_size = static_cast<int32_t>(iv);
    c = cursor(3);
    c.take(&S.n_slots, 8); c.take(&S.n_alive, 8); c.take(&S.n_edges, 8); c.take(&S.last, 8); c.take(&S.n_running, 8); c.take(&S.n_loc, 8);
  }
  const int64_t nb = S.laser.n_beams;
  if (S.n_slots < 0 || S.n_slots > INT32_MAX || S.n_alive < 0 || S.n_alive > S.n_slots || S.n_edges < 0 || S.last < -1 || S.last >= S.n_slots ||
    S.n_running < 0 || S.n_running > S.n_alive || S.n_loc < 0 || S.n_loc > S.n_alive) {return bad_file("scan counts out of range");}
  // RUNB: running[n_running], loc[n_loc] (int32), padded
  if (len[4] != round8(4 * static_cast<uint64_t>(S.n_running + S.n_loc))) {return misfit(4);}
  {Cursor c = cursor(4); if (!c.vec(S.running, S.n_running) || !c.vec(S.loc, S.n_loc)) {return misfit(4);}}
  // SCAN: per scan alive, ascending id: i32 id, i32 0, f64 time, odometric pose, corrected pose, score = 72 bytes
  if (static_cast<u128>(S.n_alive) * 72 != len[5]) {return misfit(5);}
  if (static_cast<u128>(S.n_alive) * static_cast<u128>(nb) * 8 != len[6]) {return misfit(6);}
  {
    Cursor c = cursor(5);
    const size_t n = static_cast<size_t>(S.n_alive);
    S.ids.resize(n); S.time.resize(n); S.odom.resize(3 * n); S.corr.resize(3 * n); S.score.resize(n);
    for (size_t k = 0; k < n; ++k) {
      int32_t zero = 0;
      if (!c.take(&S.ids[k], 4) || !c.take(&zero, 4) || !c.take(&S.time[k], 8) || !c.take(&S.odom[3 * k], 24) || !c.take(&S.corr[3 * k], 24) ||
        !c.take(&S.score[k], 8)) {return misfit(5);}
      if (S.ids[k] < 0 || S.ids[k] >= S.n_slots || (k > 0 && S.ids[k] <= S.ids[k - 1])) {return bad_file("scan ids are not ascending ids below the slot count");}
    }
    c = cursor(6);
    if (!c.vec(S.ranges, static_cast<uint64_t>(S.n_alive) * static_cast<uint64_t>(nb))) {return misfit(6);}
  }
  std::vector<uint8_t> is_alive(static_cast<size_t>(S.n_slots), 0);
  for (int32_t id : S.ids) {is_alive[id] = 1;}
  auto alive_id = [&](int64_t id) {return id >= 0 && id < S.n_slots && is_alive[static_cast<size_t>(id)];};
  if (S.last >= 0 && !alive_id(S.last)) {return bad_file("the last scan is not in the map");}
  for (int32_t r : S.running) {if (!alive_id(r)) {return bad_file("a running scan is not in the map");}}
  for (int32_t r : S.loc) {if (!alive_id(r)) {return bad_file("a buffered scan is not in the map");}}
  // ADJL: adj_count[n_slots], out_count[n_slots], adj[], out[] (int32), padded
  {
    if (static_cast<u128>(S.n_slots) * 8 > len[7]) {return misfit(7);}
    Cursor c = cursor(7);
    if (!c.vec(S.adj_count, S.n_slots) || !c.vec(S.out_count, S.n_slots)) {return misfit(7);}
    u128 n_adj = 0, n_out = 0;
    for (int64_t i = 0; i < S.n_slots; ++i) {
      if (S.adj_count[i] < 0 || S.out_count[i] < 0 || (!is_alive[i] && (S.adj_count[i] || S.out_count[i]))) {return bad_file("adjacency counts of a removed scan");}
      n_adj += static_cast<uint32_t>(S.adj_count[i]); n_out += static_cast<uint32_t>(S.out_count[i]);
    }
    if (round8(static_cast<uint64_t>((static_cast<u128>(S.n_slots) * 2 + n_adj + n_out) * 4)) != len[7] || (static_cast<u128>(S.n_slots) * 2 + n_adj + n_out) * 4 > len[7]) {
      return misfit(7);
    }
    if (!c.vec(S.adj, static_cast<uint64_t>(n_adj)) || !c.vec(S.out, static_cast<uint64_t>(n_out))) {return misfit(7);}
    for (int32_t a : S.adj) {if (!alive_id(a)) {return bad_file("an adjacent scan is not in the map");}}
    for (int32_t a : S.out) {if (!alive_id(a)) {return bad_file("an edge target is not in the map");}}
  }
  // SNOD: i64 n, 7 words of gauge + analysis cache, i32 id[n] padded, f64 pose[3n]
  {
    Cursor c = cursor(8);
    if (!c.take(&S.n_nodes, 8) || !c.take(S.words, 56)) {return misfit(8);}
    if (S.n_nodes < 0 || static_cast<u128>(64) + round8(4 * static_cast<uint64_t>(std::min<int64_t>(S.n_nodes, INT32_MAX))) + static_cast<u128>(S.n_nodes) * 24 != len[8] ||
      S.n_nodes > INT32_MAX) {return misfit(8);}
    if (!c.vec(S.node_ids, S.n_nodes) || !c.skip(static_cast<size_t>(round8(4 * S.n_nodes) - 4 * S.n_nodes)) || !c.vec(S.node_poses, 3 * static_cast<uint64_t>(S.n_nodes))) {return misfit(8);}
  }
  std::vector<int32_t> sorted_nodes = S.node_ids;
  std::sort(sorted_nodes.begin(), sorted_nodes.end());
  if (std::adjacent_find(sorted_nodes.begin(), sorted_nodes.end()) != sorted_nodes.end()) {return bad_file("duplicate solver node");}
  auto known_node = [&](int32_t id) {return std::binary_search(sorted_nodes.begin(), sorted_nodes.end(), id);};
  // SCON: i64 m, i32 a[m], i32 b[m], f64 z[3m], f64 info[6m]
  {
    Cursor c = cursor(9);
    if (!c.take(&S.n_cons, 8)) {return misfit(9);}
    if (S.n_cons < 0 || S.n_cons > INT32_MAX || static_cast<u128>(8) + static_cast<u128>(S.n_cons) * (8 + 24 + 48) != len[9]) {return misfit(9);}
    if (!c.vec(S.ca, S.n_cons) || !c.vec(S.cb, S.n_cons) || !c.vec(S.cz, 3 * static_cast<uint64_t>(S.n_cons)) || !c.vec(S.cinfo, 6 * static_cast<uint64_t>(S.n_cons))) {return misfit(9);}
    for (int64_t k = 0; k < S.n_cons; ++k) {
      if (S.ca[k] == S.cb[k] || !known_node(S.ca[k]) || !known_node(S.cb[k])) {return bad_file("a constraint between unknown solver nodes");}
    }
  }
  // SANA: i64 n_supernodes, i32 ptr[n + 1], i32 ids[ptr[n]], padded
  {
    Cursor c = cursor(10);
    if (!c.take(&S.n_sn, 8)) {return misfit(10);}
    if (S.n_sn < 0 || static_cast<u128>(S.n_sn) * 4 + 12 > len[10]) {return misfit(10);}
    if (!c.vec(S.sn_ptr, static_cast<uint64_t>(S.n_sn) + 1)) {return misfit(10);}
    if (S.sn_ptr[0] != 0) {return misfit(10);}
    for (int64_t k = 0; k < S.n_sn; ++k) {if (S.sn_ptr[k + 1] < S.sn_ptr[k]) {return misfit(10);}}
    const uint64_t total = static_cast<uint64_t>(S.sn_ptr[static_cast<size_t>(S.n_sn)]);
    if (round8(8 + 4 * (static_cast<uint64_t>(S.n_sn) + 1 + total)) != len[10]) {return misfit(10);}
    if (!c.vec(S.sn_ids, total)) {return misfit(10);}
  }
  return KH_OK;
}

int load_and_parse(const char * path, Session & S)
{
  std::string data;
  if (!read_file(path, data)) {return bad_file(std::string("cannot read ") + path);}
  return parse_session(data, S);
}
}  // namespace
}  // namespace mapper
}  // namespace kh

using namespace kh;
using namespace kh::mapper;

extern "C" {

int kh_mapper_save(const kh_mapper * m, const char * path)
{
  if (!m || !path) {return KH_ERR_INVALID_ARG;}
  if (m->failed) {
    set_error("kh_mapper_save: an earlier Process() failed after its scan had entered the graph; the state is not a run's state");
    return KH_ERR_INVALID_ARG;
  }
  Blob sec[kSections];
  {
    const kh_mapper_params & p = m->p;
#define KH_WR_I(f) sec[0].i64(p.f);
#define KH_WR_D(f) sec[0].f64(p.f);
    KH_SESSION_PARAM_WORDS(KH_WR_I, KH_WR_D)
#undef KH_WR_I
#undef KH_WR_D
  }
  const kh_laser L = to_kh_laser(m->laser);           // (the fields in the order parse_session reads them)
  sec[1].i64(L.n_beams); sec[1].f64(L.minimum_angle); sec[1].f64(L.angular_resolution); sec[1].f64(L.minimum_range); sec[1].f64(L.maximum_range);
  sec[1].f64(L.range_threshold); sec[1].f64(L.offset_x); sec[1].f64(L.offset_y); sec[1].f64(L.offset_heading);
  kh_decay_params d;
  std::memset(&d, 0, sizeof(d));
  if (m->lifelong) {d = m->decay;}
  sec[2].i64(m->lifelong ? 1 : 0);
  sec[2].f64(d.iou_thresh); sec[2].f64(d.iou_match); sec[2].f64(d.removal_score); sec[2].f64(d.overlap_scale); sec[2].f64(d.constraint_scale);
  sec[2].f64(d.nearby_penalty); sec[2].f64(d.candidates_scale); sec[2].i64(d.scan_buffer_size);
  int64_t n_alive = 0;
  for (const auto & s : m->scans) {n_alive += s ? 1 : 0;}
  sec[3].i64(static_cast<int64_t>(m->scans.size())); sec[3].i64(n_alive); sec[3].i64(m->n_edges); sec[3].i64(m->last);
  sec[3].i64(static_cast<int64_t>(m->running.size())); sec[3].i64(static_cast<int64_t>(m->loc_buffer.size()));
  sec[4].i32s(m->running); sec[4].i32s(m->loc_buffer); sec[4].pad8();
  sec[5].b.reserve(static_cast<size_t>(n_alive) * 72); sec[6].b.reserve(static_cast<size_t>(n_alive) * 8 * static_cast<size_t>(L.n_beams));
  for (const auto & sp : m->scans) {
    if (!sp) {continue;}
    const MScan & s = *sp;
    const int32_t head[2] = {s.id, 0};
    double poses[6];
    put_pose(s.odometric, poses); put_pose(s.corrected, poses + 3);
    sec[5].raw(head, 8); sec[5].f64(s.time); sec[5].raw(poses, 48); sec[5].f64(s.score);
    sec[6].raw(s.ranges.data(), 8 * s.ranges.size());
  }
  {
    std::vector<int32_t> counts;
    for (const auto & a : m->adj) {counts.push_back(static_cast<int32_t>(a.size()));}
    sec[7].i32s(counts);
    counts.clear();
    for (const auto & a : m->out_edges) {counts.push_back(static_cast<int32_t>(a.size()));}
    sec[7].i32s(counts);
    for (const auto & a : m->adj) {sec[7].i32s(a);}
    for (const auto & a : m->out_edges) {sec[7].i32s(a);}
    sec[7].pad8();
  }
  {
    int64_t words[7];
    std::vector<int32_t> sn_ptr, sn_ids;
    spa_export_session_state(m->solver, words, sn_ptr, sn_ids);
    const int32_t n = kh_spa_num_nodes(m->solver), nc = kh_spa_num_constraints(m->solver);
    std::vector<int32_t> ids(static_cast<size_t>(n));
    std::vector<double> poses(3 * static_cast<size_t>(n));
    if (n) {kh_spa_get_nodes(m->solver, ids.data(), poses.data());}
    sec[8].i64(n); sec[8].raw(words, 56); sec[8].i32s(ids); sec[8].pad8();
    if (n) {sec[8].raw(poses.data(), 8 * poses.size());}
    std::vector<int32_t> ca(static_cast<size_t>(nc)), cb(static_cast<size_t>(nc));
    std::vector<double> cz(3 * static_cast<size_t>(nc)), ci(6 * static_cast<size_t>(nc));
    for (int32_t k = 0; k < nc; ++k) {
      const int rc = kh_spa_get_constraint(m->solver, k, &ca[k], &cb[k], &cz[3 * k], &ci[6 * k]);
      if (rc) {return rc;}
    }
    sec[9].i64(nc); sec[9].i32s(ca); sec[9].i32s(cb);
    if (nc) {sec[9].raw(cz.data(), 8 * cz.size()); sec[9].raw(ci.data(), 8 * ci.size());}
    sec[10].i64(static_cast<int64_t>(sn_ptr.size()) - 1); sec[10].i32s(sn_ptr); sec[10].i32s(sn_ids); sec[10].pad8();
  }
  std::string body;                                  // section table + sections = what the checksum covers
  uint64_t at = kHeaderBytes + kTableBytes;
  for (int k = 0; k < kSections; ++k) {
    const uint32_t zero = 0;
    const uint64_t len = sec[k].b.size();
    body.append(kSectionTags[k], 4); body.append(reinterpret_cast<const char *>(&zero), 4);
    body.append(reinterpret_cast<const char *>(&at), 8); body.append(reinterpret_cast<const char *>(&len), 8);
    at += len;
  }
  for (int k = 0; k < kSections; ++k) {body += sec[k].b; sec[k].b.clear(); sec[k].b.shrink_to_fit();}
  const uint32_t version = kSessionVersion, n_sections = kSections;
  const uint32_t crc = crc32_ieee(reinterpret_cast<const uint8_t *>(body.data()), body.size());
  FILE * f = std::fopen(path, "wb");
  if (!f) {set_error("kh_mapper_save: cannot open the file for writing"); return KH_ERR_IO;}
  bool ok = std::fwrite("KHMS", 1, 4, f) == 4 && std::fwrite(&version, 4, 1, f) == 1 && std::fwrite(&at, 8, 1, f) == 1 &&
    std::fwrite(&n_sections, 4, 1, f) == 1 && std::fwrite(&crc, 4, 1, f) == 1 && std::fwrite(body.data(), 1, body.size(), f) == body.size();
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) {set_error("kh_mapper_save: write failed"); return KH_ERR_IO;}
  return KH_OK;
}

int kh_session_info(const char * path, kh_session_info_t * out)
{
  if (!path || !out) {return KH_ERR_INVALID_ARG;}
  Session S;
  const int rc = load_and_parse(path, S);
  if (rc) {return rc;}
  out->version = S.version; out->file_bytes = S.file_bytes; out->n_beams = S.laser.n_beams; out->n_scan_slots = S.n_slots; out->n_alive = S.n_alive;
  out->n_edges = S.n_edges; out->n_running = S.n_running; out->last_scan = S.last; out->n_localization_buffer = S.n_loc; out->lifelong = S.lifelong;
  out->n_solver_nodes = S.n_nodes; out->n_solver_constraints = S.n_cons; out->n_supernodes = S.n_sn;
  return KH_OK;
}

int kh_mapper_load(const char * path, const int32_t * devices, int32_t n_devices, int32_t max_candidates, kh_mapper ** out)
{
  if (!path || !out || !devices || n_devices < 1 || max_candidates < 1) {return KH_ERR_INVALID_ARG;}
  *out = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  Session S;
  int rc = load_and_parse(path, S);                 // the whole file is validated before a device is touched
  if (rc) {return rc;}
  const auto t1 = std::chrono::steady_clock::now();
  kh_mapper * m = nullptr;
  rc = kh_mapper_create_on_devices(&S.p, &S.laser, devices, n_devices, max_candidates, &m);
  if (rc) {return rc;}
  auto fail = [&](int code) {kh_mapper_destroy(m); return code;};
  if (S.lifelong) {m->lifelong = true; m->decay = S.decay;}
  const size_t nb = static_cast<size_t>(S.laser.n_beams);
  m->scans.resize(static_cast<size_t>(S.n_slots));
  for (size_t k = 0; k < S.ids.size(); ++k) {
    std::unique_ptr<MScan> s(new MScan());
    s->id = S.ids[k]; s->time = S.time[k]; s->score = S.score[k];
    s->odometric = to_pose(&S.odom[3 * k]); s->corrected = to_pose(&S.corr[3 * k]);
    s->ranges.assign(S.ranges.begin() + static_cast<std::ptrdiff_t>(k * nb), S.ranges.begin() + static_cast<std::ptrdiff_t>((k + 1) * nb));
    m->scans[static_cast<size_t>(S.ids[k])] = std::move(s);
  }
  // LocalizedRangeScan::Update of every scan: N x P glibc sincos, on the host pools like CorrectPoses
  update_scans_bulk(S.ids.size(), [&](size_t k) {update_scan(*m->scans[static_cast<size_t>(S.ids[k])], m->laser);});
  const auto t2 = std::chrono::steady_clock::now();
  m->adj.assign(static_cast<size_t>(S.n_slots), {}); m->out_edges.assign(static_cast<size_t>(S.n_slots), {});
  {
    size_t a = 0, o = 0;
    for (size_t i = 0; i < static_cast<size_t>(S.n_slots); ++i) {
      m->adj[i].assign(S.adj.begin() + static_cast<std::ptrdiff_t>(a), S.adj.begin() + static_cast<std::ptrdiff_t>(a + S.adj_count[i])); a += S.adj_count[i];
    }
    for (size_t i = 0; i < static_cast<size_t>(S.n_slots); ++i) {
      m->out_edges[i].assign(S.out.begin() + static_cast<std::ptrdiff_t>(o), S.out.begin() + static_cast<std::ptrdiff_t>(o + S.out_count[i])); o += S.out_count[i];
    }
  }
  m->n_edges = S.n_edges; m->running = S.running; m->loc_buffer = S.loc; m->last = static_cast<int32_t>(S.last);
  // the solver: Reset, AddNode*, AddConstraint* in the stored order with the stored information matrices (loadSerializedPoseGraph,
  // slam_toolbox_common.cpp:959-1016), then the gauge and the analysis cache as they stood.  No Compute(): see DESIGN.md section 7
  kh_spa_reset(m->solver);
  for (int64_t k = 0; k < S.n_nodes; ++k) {
    rc = kh_spa_add_node(m->solver, S.node_ids[k], &S.node_poses[3 * k]);
    if (rc) {return fail(rc);}
  }
  for (int64_t k = 0; k < S.n_cons; ++k) {
    rc = kh_spa_add_constraint_information(m->solver, S.ca[k], S.cb[k], &S.cz[3 * k], &S.cinfo[6 * k]);
    if (rc) {bad_file("a constraint's information matrix is not positive definite"); return fail(KH_ERR_IO);}
  }
  spa_import_session_state(m->solver, S.words, S.sn_ptr, S.sn_ids);
  const auto t3 = std::chrono::steady_clock::now();
  m->graph_dirty = true;
  rc = sync_graph(m);
  if (rc) {return fail(rc);}
  const auto t4 = std::chrono::steady_clock::now();
  g_last_load_ms[0] = ms_between(t0, t1); g_last_load_ms[1] = ms_between(t1, t2); g_last_load_ms[2] = ms_between(t2, t3); g_last_load_ms[3] = ms_between(t3, t4);
  *out = m;
  return KH_OK;
}

int kh_session_last_load_ms(double out[4])
{
  if (!out) {return KH_ERR_INVALID_ARG;}
  std::copy(g_last_load_ms, g_last_load_ms + 4, out);
  return KH_OK;
}

}  // extern "C"
