// wbc_urdf.h -- URDF -> wbc_model on the host (wbc_asset_load_urdf, include/wbc_sim.h). Header-only, plain C++17, no HIP: wbc_sim.hip
// includes it next to the .wbcasset loader, and the CPU tests build it alone with g++ and sanitizers.
//
// Two parts. A small XML reader: the declaration, comments, CDATA, self-closing tags, attributes in either quote, the five
// predefined entities and character references; anything else is an error with its line number. Then the model build, restated
// from the Python host path: urdf_model.parse_urdf + build_model and abi.collision_set +
// quantise_reach + fill_model. Every floating-point step is the same double-precision operation in the same order, so the floats
// stored into wbc_model round from the same doubles. numpy's 3x3 products (R I R^T, rpy_to_mat) and 3-vector dot products go
// through OpenBLAS, whose kernels accumulate with fused multiply-adds in ascending k: mat3 / dot3 below do the same.
#pragma once

#include <algorithm>
#include <array>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/wbc_sim.h"

// No a*b+c below may become a fused multiply-add (numpy rounds every product): the arithmetic functions open with this. Block-scoped,
// so the kernels of the file that includes this header keep their own contraction setting.
#if defined(__clang__)
#define WBC_URDF_NO_FMA_CONTRACTION _Pragma("clang fp contract(off)")
#else
#define WBC_URDF_NO_FMA_CONTRACTION
#endif

namespace wbc_urdf {

enum { kMalformed = -2, kUnsupported = -4 };

// ---- XML -----------------------------------------------------------------------------------------------------------------------
struct Node {
  std::string name;
  std::vector<std::pair<std::string, std::string>> attrs;
  std::vector<Node> kids;
  int line = 0;
  const std::string* attr(const char* k) const {
    for (const auto& a : attrs)
      if (a.first == k) return &a.second;
    return nullptr;
  }
  const Node* child(const char* n) const {   // ElementTree.find: the first direct child of that name
    for (const auto& c : kids)
      if (c.name == n) return &c;
    return nullptr;
  }
};

class XmlReader {
 public:
  XmlReader(const std::string& text, std::string& err) : s_(text), err_(err) {}

  int parse(Node& root) {
    if (!misc()) return kMalformed;
    if (at_end() || s_[p_] != '<') return fail("expected the root element");
    std::vector<Node*> stack;
    bool closed = false;
    if (!start_tag(root, closed)) return kMalformed;
    if (!closed) stack.push_back(&root);
    while (!stack.empty()) {
      if (at_end()) return fail("unexpected end of file inside <" + stack.back()->name + "> opened at line " + std::to_string(stack.back()->line));
      if (s_[p_] != '<') {
        if (!text()) return kMalformed;
      } else if (starts("<!--")) {
        if (!comment()) return kMalformed;
      } else if (starts("<![CDATA[")) {
        if (!skip_past("]]>", "CDATA section")) return kMalformed;
      } else if (starts("<?")) {
        if (!skip_past("?>", "processing instruction")) return kMalformed;
      } else if (starts("</")) {
        int l = line_;
        adv(2);
        std::string n;
        if (!name(n)) return kMalformed;
        ws();
        if (at_end() || s_[p_] != '>') return fail("expected '>' after </" + n);
        adv(1);
        Node* open = stack.back();
        if (n != open->name) return fail_at(l, "</" + n + "> closes <" + open->name + "> opened at line " + std::to_string(open->line));
        stack.pop_back();
      } else {
        if (stack.size() >= kMaxDepth) return fail("elements nested deeper than " + std::to_string(kMaxDepth));
        Node* parent = stack.back();
        parent->kids.emplace_back();
        Node* kid = &parent->kids.back();
        if (!start_tag(*kid, closed)) return kMalformed;
        if (!closed) stack.push_back(kid);   // ancestors' vectors do not grow while a descendant is open: the pointers stay valid
      }
    }
    if (!misc()) return kMalformed;
    if (!at_end()) return fail("content after the root element </" + root.name + ">");
    return 0;
  }

 private:
  static constexpr size_t kMaxDepth = 256;
  const std::string& s_;
  std::string& err_;
  size_t p_ = 0;
  int line_ = 1;

  bool at_end() const { return p_ >= s_.size(); }
  bool starts(const char* lit) const { return s_.compare(p_, strlen(lit), lit) == 0; }
  void adv(size_t n) {
    for (size_t e = std::min(s_.size(), p_ + n); p_ < e; ++p_)
      if (s_[p_] == '\n') ++line_;
  }
  int fail_at(int line, const std::string& msg) { err_ = "line " + std::to_string(line) + ": " + msg; return kMalformed; }
  int fail(const std::string& msg) { return fail_at(line_, msg); }
  static bool is_ws(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
  void ws() { while (!at_end() && is_ws(s_[p_])) adv(1); }
  bool skip_past(const char* term, const char* what) {
    size_t e = s_.find(term, p_);
    if (e == std::string::npos) { fail(std::string("unexpected end of file in a ") + what); return false; }
    adv(e + strlen(term) - p_);
    return true;
  }
  bool comment() { adv(4); return skip_past("-->", "comment"); }
  // whitespace, comments, processing instructions (the XML declaration) and a DOCTYPE around the root element
  bool misc() {
    for (;;) {
      ws();
      if (starts("<!--")) { if (!comment()) return false; }
      else if (starts("<?")) { if (!skip_past("?>", "processing instruction")) return false; }
      else if (starts("<!DOCTYPE")) { if (!skip_past(">", "DOCTYPE")) return false; }
      else return true;
    }
  }
  static bool name_start(unsigned char c) { return isalpha(c) || c == '_' || c == ':' || c >= 0x80; }
  static bool name_char(unsigned char c) { return name_start(c) || isdigit(c) || c == '-' || c == '.'; }
  bool name(std::string& out) {
    if (at_end() || !name_start((unsigned char)s_[p_])) { fail("expected a name"); return false; }
    size_t b = p_;
    while (!at_end() && name_char((unsigned char)s_[p_])) ++p_;
    out.assign(s_, b, p_ - b);
    return true;
  }
  static void utf8(uint32_t cp, std::string& out) {
    if (cp < 0x80) { out += (char)cp; }
    else if (cp < 0x800) { out += (char)(0xC0 | (cp >> 6)); out += (char)(0x80 | (cp & 0x3F)); }
    else if (cp < 0x10000) { out += (char)(0xE0 | (cp >> 12)); out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F)); }
    else { out += (char)(0xF0 | (cp >> 18)); out += (char)(0x80 | ((cp >> 12) & 0x3F)); out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F)); }
  }
  // at '&': append the character it stands for
  bool entity(std::string& out) {
    size_t e = s_.find(';', p_);
    if (e == std::string::npos || e - p_ > 12) { fail("unterminated entity reference"); return false; }
    std::string ent(s_, p_ + 1, e - p_ - 1);
    static const char* const kNames[5] = {"lt", "gt", "amp", "quot", "apos"};
    static const char kChars[5] = {'<', '>', '&', '"', '\''};
    for (int i = 0; i < 5; ++i)
      if (ent == kNames[i]) { out += kChars[i]; adv(e + 1 - p_); return true; }
    if (ent.size() >= 2 && ent[0] == '#') {
      bool hex = ent[1] == 'x';
      const char* d = ent.c_str() + (hex ? 2 : 1);
      char* end = nullptr;
      unsigned long cp = (*d && isxdigit((unsigned char)*d)) ? strtoul(d, &end, hex ? 16 : 10) : 0;
      if (end && *end == 0 && cp > 0 && cp <= 0x10FFFF) { utf8((uint32_t)cp, out); adv(e + 1 - p_); return true; }
    }
    fail("unknown entity &" + ent + ";");
    return false;
  }
  bool text() {   // character data between tags: not stored (URDF keeps everything in attributes), but its entities are checked
    std::string sink;
    while (!at_end() && s_[p_] != '<') {
      if (s_[p_] == '&') { if (!entity(sink)) return false; sink.clear(); }
      else adv(1);
    }
    return true;
  }
  bool start_tag(Node& n, bool& closed) {
    n.line = line_;
    adv(1);
    if (!name(n.name)) return false;
    for (;;) {
      size_t before = p_;
      ws();
      if (at_end()) { fail("unexpected end of file in <" + n.name + ">"); return false; }
      if (s_[p_] == '>') { adv(1); closed = false; return true; }
      if (starts("/>")) { adv(2); closed = true; return true; }
      if (p_ == before) { fail("expected whitespace, '>' or '/>' in <" + n.name + ">"); return false; }
      std::string k, v;
      if (!name(k)) return false;
      ws();
      if (at_end() || s_[p_] != '=') { fail("attribute " + k + " of <" + n.name + "> has no value"); return false; }
      adv(1);
      ws();
      if (at_end() || (s_[p_] != '"' && s_[p_] != '\'')) { fail("attribute " + k + " of <" + n.name + ">: expected a quoted value"); return false; }
      char q = s_[p_];
      adv(1);
      while (!at_end() && s_[p_] != q) {
        if (s_[p_] == '<') { fail("'<' in the value of attribute " + k); return false; }
        if (s_[p_] == '&') { if (!entity(v)) return false; }
        else { v += s_[p_]; adv(1); }
      }
      if (at_end()) { fail("unexpected end of file in the value of attribute " + k + " of <" + n.name + ">"); return false; }
      adv(1);
      if (n.attr(k.c_str())) { fail("duplicate attribute " + k + " in <" + n.name + ">"); return false; }
      n.attrs.emplace_back(std::move(k), std::move(v));
    }
  }
};

// ---- numbers and small linear algebra (double, in numpy's order) ---------------------------------------------------------------
using Vec3 = std::array<double, 3>;
using Mat3 = std::array<Vec3, 3>;

// whitespace-separated decimal numbers (Python's float() on str.split(); strtod rounds the same way)
inline bool parse_numbers(const std::string& s, double* out, int n) {
  const char* c = s.c_str();
  for (int i = 0; i < n; ++i) {
    while (*c == ' ' || *c == '\t' || *c == '\n' || *c == '\r') ++c;
    if (!*c) return false;
    char* end = nullptr;
    out[i] = strtod(c, &end);
    if (end == c || (*end && *end != ' ' && *end != '\t' && *end != '\n' && *end != '\r')) return false;
    c = end;
  }
  while (*c == ' ' || *c == '\t' || *c == '\n' || *c == '\r') ++c;
  return *c == 0;
}

inline Mat3 mat3(const Mat3& a, const Mat3& b) {   // numpy a @ b (OpenBLAS dgemm: acc = fma(a_ik, b_kj, acc), k ascending)
  Mat3 r{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) acc = std::fma(a[i][k], b[k][j], acc);
      r[i][j] = acc;
    }
  return r;
}
inline Mat3 transpose(const Mat3& a) {
  Mat3 r{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[i][j] = a[j][i];
  return r;
}
inline double dot3(const Vec3& a, const Vec3& b) {   // numpy np.dot of two 3-vectors (OpenBLAS ddot)
  double acc = 0.0;
  for (int k = 0; k < 3; ++k) acc = std::fma(a[k], b[k], acc);
  return acc;
}
inline Vec3 add(const Vec3& a, const Vec3& b) { return {a[0] + b[0], a[1] + b[1], a[2] + b[2]}; }
inline Vec3 sub(const Vec3& a, const Vec3& b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }

inline Mat3 rpy_to_mat(const Vec3& rpy) {   // urdf_model.rpy_to_mat: Rz @ Ry @ Rx
  double cr = cos(rpy[0]), sr = sin(rpy[0]), cp = cos(rpy[1]), sp = sin(rpy[1]), cy = cos(rpy[2]), sy = sin(rpy[2]);
  Mat3 Rx{{{1, 0, 0}, {0, cr, -sr}, {0, sr, cr}}};
  Mat3 Ry{{{cp, 0, sp}, {0, 1, 0}, {-sp, 0, cp}}};
  Mat3 Rz{{{cy, -sy, 0}, {sy, cy, 0}, {0, 0, 1}}};
  return mat3(mat3(Rz, Ry), Rx);
}

// I + mm * (|d|^2 E - d d^T), elementwise as numpy evaluates it
inline Mat3 shift(const Mat3& I, double mm, const Vec3& d) {
  WBC_URDF_NO_FMA_CONTRACTION
  double dd = dot3(d, d);
  Mat3 r{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[i][j] = I[i][j] + mm * (dd * (i == j ? 1.0 : 0.0) - d[i] * d[j]);
  return r;
}

struct Body { double m = 0.0; Vec3 c{}; Mat3 I{}; };

inline Body merge(const Body& a, double m2, const Vec3& c2, const Mat3& I2) {   // urdf_model._merge
  WBC_URDF_NO_FMA_CONTRACTION
  Body r;
  r.m = a.m + m2;
  if (r.m <= 0.0) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r.I[i][j] = a.I[i][j] + I2[i][j];
    return r;
  }
  for (int i = 0; i < 3; ++i) r.c[i] = (a.m * a.c[i] + m2 * c2[i]) / r.m;
  Mat3 s1 = shift(a.I, a.m, sub(a.c, r.c)), s2 = shift(I2, m2, sub(c2, r.c));
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.I[i][j] = s1[i][j] + s2[i][j];
  return r;
}

inline Body unmerge(const Body& t, const Body& p) {   // urdf_model._unmerge: `t` without `p`
  WBC_URDF_NO_FMA_CONTRACTION
  Body r;
  r.m = t.m - p.m;
  if (r.m <= 1e-12) { r.m = 0.0; r.c = t.c; return r; }
  for (int i = 0; i < 3; ++i) r.c[i] = (t.m * t.c[i] - p.m * p.c[i]) / r.m;
  Mat3 sp = shift(p.I, p.m, sub(p.c, t.c));
  Vec3 d = sub(r.c, t.c);
  double dd = dot3(d, d);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.I[i][j] = t.I[i][j] - sp[i][j] - r.m * (dd * (i == j ? 1.0 : 0.0) - d[i] * d[j]);
  return r;
}

inline void sym6(const Mat3& I, float* out) {
  const double v[6] = {I[0][0], I[1][1], I[2][2], I[0][1], I[0][2], I[1][2]};
  for (int i = 0; i < 6; ++i) out[i] = (float)v[i];
}
inline void put3(float* out, const Vec3& v) { for (int i = 0; i < 3; ++i) out[i] = (float)v[i]; }

// ---- URDF tables ---------------------------------------------------------------------------------------------------------------
struct Link { std::string name; double mass = 0.0; Vec3 com{}; Mat3 inertia{}; int line = 0; };
struct Joint {
  std::string name, type, parent, child;
  Vec3 xyz{}, rpy{}, axis{{1.0, 0.0, 0.0}};
  double lower = 0.0, upper = 0.0, velocity = 0.0, effort = 0.0, friction = 0.0, damping = 0.0;
  bool dont_collapse = false;
  int line = 0;
};

// what the loader hands to wbc_asset: the model, the names, the URDF's DoF properties (as doubles, for the soft limits)
struct Result {
  wbc_model model;
  std::vector<std::string> dof_names, rb_names;
  std::vector<wbc_dof_props> props;
  std::vector<double> lower, upper, velocity, effort;
};

inline void default_opts(wbc_asset_opts* o) {   // the shipped WidowGo1RoughCfg (widowGo1_config.py) and abi.ARM_LIMB_FIT
  memset(o, 0, sizeof(*o));
  o->struct_size = (uint32_t)sizeof(wbc_asset_opts);
  o->default_dof_drive_mode = 3;
  o->collapse_fixed_joints = 1;
  o->replace_cylinder_with_capsule = 1;
  o->density = 0.001;
  o->max_angular_velocity = 1000.0;
  o->max_linear_velocity = 1000.0;
  o->thickness = 0.01;
  o->self_collisions = 0;
  snprintf(o->root_link, sizeof(o->root_link), "%s", "base");
  snprintf(o->foot_name, sizeof(o->foot_name), "%s", "foot");
  snprintf(o->gripper_name, sizeof(o->gripper_name), "%s", "wx250s/ee_gripper_link");
  o->lock_friction_above = 100.0;
  o->box_size = 0.1;
  o->rest_offset = 0.0;
  const double fit[3][3] = {{0.04, 0.0, 0.0}, {0.025, 0.0, 0.0}, {0.0275, 0.0, 0.0}};   // "balanced" fit, rounded to 0.1 mm
  memcpy(o->arm_limb_fit, fit, sizeof(fit));
  o->soft_dof_pos_limit = o->soft_dof_vel_limit = o->soft_torque_limit = 1.0;
}

// the asset.* rows of abi.UNSUPPORTED_SWITCHES, plus the struct's own consistency
inline int check_opts(const wbc_asset_opts& o, std::string& err) {
  if (o.struct_size != sizeof(wbc_asset_opts)) {
    err = "wbc_asset_opts.struct_size is " + std::to_string(o.struct_size) + ", this library's is " + std::to_string(sizeof(wbc_asset_opts)) +
          " (call wbc_asset_opts_default first)";
    return -1;
  }
  for (const char* s : {o.root_link, o.foot_name, o.gripper_name})
    if (!memchr(s, 0, 64) || !s[0]) { err = "wbc_asset_opts: root_link / foot_name / gripper_name must be non-empty, NUL-terminated"; return -1; }
  if (o.fix_base_link) { err = "wbc_asset_opts.fix_base_link = 1: the physics is a floating base (DESIGN.md section 3)"; return kUnsupported; }
  if (o.disable_gravity) { err = "wbc_asset_opts.disable_gravity = 1: not modelled; set wbc_task_cfg.gravity instead"; return kUnsupported; }
  if (!o.collapse_fixed_joints) { err = "wbc_asset_opts.collapse_fixed_joints = 0: the rigid-body list (27 bodies, quirk Q1) is the collapsed one"; return kUnsupported; }
  if (o.default_dof_drive_mode != 3) {
    err = "wbc_asset_opts.default_dof_drive_mode = " + std::to_string(o.default_dof_drive_mode) + ": the task drives joints by effort (3, WG:1183)";
    return kUnsupported;
  }
  if (o.linear_damping != 0.0) { err = "wbc_asset_opts.linear_damping != 0: body damping is not modelled"; return kUnsupported; }
  if (o.angular_damping != 0.0) { err = "wbc_asset_opts.angular_damping != 0: body damping is not modelled"; return kUnsupported; }
  return 0;
}

class Loader {
 public:
  Loader(const wbc_asset_opts& o, Result& out, std::string& err) : o_(o), out_(out), err_(err) {}

  int run(const std::string& text) {
    Node root;
    int rc = XmlReader(text, err_).parse(root);
    if (rc) return rc;
    if (root.name != "robot") return bad(kMalformed, "the root element is <" + root.name + ">, not <robot>");
    if ((rc = tables(root))) return rc;
    if ((rc = build())) return rc;
    if ((rc = fill())) return rc;
    return 0;
  }

 private:
  const wbc_asset_opts& o_;
  Result& out_;
  std::string& err_;
  std::vector<Link> links_;
  std::map<std::string, int> link_of_;
  std::vector<Joint> joints_;
  std::map<std::string, std::vector<int>> children_;
  // build_model's lists
  std::vector<int> parent_, axis_, body_dof_, dof_joint_, rb_body_;
  std::vector<bool> dof_locked_;
  std::vector<Vec3> joint_xyz_, rb_offset_;
  std::vector<Body> comp_;
  std::vector<std::string> rb_names_;
  std::set<std::string> visited_;
  Body base_piece_, base_rest_, grip_piece_, grip_rest_;
  static constexpr int kMaxTreeDepth = 64;   // link levels below the root (widowGo1's deepest chain: 11)
  int grip_body_ = 0;

  int bad(int code, const std::string& msg) { err_ = msg; return code; }
  static std::string at(int line) { return " (line " + std::to_string(line) + ")"; }

  int num(const Node& e, const char* key, const char* dflt, double* out, int n, const std::string& what) {
    const std::string* v = e.attr(key);
    if (!v && !dflt) return bad(kMalformed, what + at(e.line) + ": <" + e.name + "> has no " + key + " attribute");
    const std::string text = v ? *v : std::string(dflt);
    if (!parse_numbers(text, out, n))
      return bad(kMalformed, what + at(e.line) + ": <" + e.name + " " + key + "=\"" + text + "\">: expected " + std::to_string(n) + " number(s)");
    return 0;
  }

  // urdf_model.parse_urdf: direct <link> / <joint> children of <robot> (ElementTree.findall)
  int tables(const Node& root) {
    int rc;
    for (const Node& le : root.kids) {
      if (le.name != "link") continue;
      const std::string* nm = le.attr("name");
      if (!nm) return bad(kMalformed, "<link>" + at(le.line) + " has no name");
      Link lk;
      lk.name = *nm;
      lk.line = le.line;
      std::string what = "link " + lk.name;
      if (const Node* ie = le.child("inertial")) {
        const Node* me = ie->child("mass");
        const Node* ine = ie->child("inertia");
        if (!me || !ine) return bad(kMalformed, what + at(ie->line) + ": <inertial> needs <mass> and <inertia>");
        if ((rc = num(*me, "value", nullptr, &lk.mass, 1, what))) return rc;
        Vec3 xyz{}, rpy{};
        if (const Node* oe = ie->child("origin")) {
          if ((rc = num(*oe, "xyz", "0 0 0", xyz.data(), 3, what)) || (rc = num(*oe, "rpy", "0 0 0", rpy.data(), 3, what))) return rc;
        }
        double v[6];
        static const char* const kKeys[6] = {"ixx", "ixy", "ixz", "iyy", "iyz", "izz"};
        for (int i = 0; i < 6; ++i)
          if ((rc = num(*ine, kKeys[i], nullptr, &v[i], 1, what))) return rc;
        Mat3 I{{{v[0], v[1], v[2]}, {v[1], v[3], v[4]}, {v[2], v[4], v[5]}}};
        Mat3 R = rpy_to_mat(rpy);
        lk.com = xyz;
        lk.inertia = mat3(mat3(R, I), transpose(R));
      }
      if (link_of_.count(lk.name)) return bad(kMalformed, what + at(le.line) + ": a second <link> of that name");
      link_of_[lk.name] = (int)links_.size();
      links_.push_back(std::move(lk));
    }
    for (const Node& je : root.kids) {
      if (je.name != "joint") continue;
      Joint j;
      j.line = je.line;
      const std::string* nm = je.attr("name");
      const std::string* ty = je.attr("type");
      if (!nm || !ty) return bad(kMalformed, "<joint>" + at(je.line) + " needs a name and a type");
      j.name = *nm;
      j.type = *ty;
      std::string what = "joint " + j.name;
      const Node* pe = je.child("parent");
      const Node* ce = je.child("child");
      const std::string* pl = pe ? pe->attr("link") : nullptr;
      const std::string* cl = ce ? ce->attr("link") : nullptr;
      if (!pl || !cl) return bad(kMalformed, what + at(je.line) + ": needs <parent link=...> and <child link=...>");
      j.parent = *pl;
      j.child = *cl;
      for (const std::string* l : {pl, cl})
        if (!link_of_.count(*l)) return bad(kMalformed, what + at(je.line) + ": names the unknown link '" + *l + "'");
      if (const Node* oe = je.child("origin")) {
        if ((rc = num(*oe, "xyz", "0 0 0", j.xyz.data(), 3, what)) || (rc = num(*oe, "rpy", "0 0 0", j.rpy.data(), 3, what))) return rc;
      }
      if (const Node* ae = je.child("axis")) {
        if ((rc = num(*ae, "xyz", nullptr, j.axis.data(), 3, what))) return rc;
      }
      if (const Node* le = je.child("limit")) {
        if ((rc = num(*le, "lower", "0", &j.lower, 1, what)) || (rc = num(*le, "upper", "0", &j.upper, 1, what)) ||
            (rc = num(*le, "velocity", "0", &j.velocity, 1, what)) || (rc = num(*le, "effort", "0", &j.effort, 1, what)))
          return rc;
      }
      if (const Node* de = je.child("dynamics")) {
        if ((rc = num(*de, "friction", "0", &j.friction, 1, what)) || (rc = num(*de, "damping", "0", &j.damping, 1, what))) return rc;
      }
      const std::string* dc = je.attr("dont_collapse");
      j.dont_collapse = dc && *dc == "true";
      joints_.push_back(std::move(j));
    }
    for (int i = 0; i < (int)joints_.size(); ++i) children_[joints_[i].parent].push_back(i);
    for (auto& kv : children_)   // the importer's alphabetical child order (quirk Q1); Python's sort is stable
      std::stable_sort(kv.second.begin(), kv.second.end(), [this](int a, int b) { return joints_[a].child < joints_[b].child; });
    return 0;
  }

  void add_rb(const std::string& name, int body, const Vec3& off) {
    rb_names_.push_back(name);
    rb_body_.push_back(body);
    rb_offset_.push_back(off);
  }

  // build_model.visit: `link` rides on moving body `body` at translation `offset`
  int visit(const std::string& link, int body, const Vec3& offset, int depth) {
    if (depth > kMaxTreeDepth)   // bounds the recursion: every malformed tree ends in an error code, not a stack overflow
      return bad(kUnsupported, "link " + link + ": the link tree is deeper than " + std::to_string(kMaxTreeDepth) +
                               " levels (the kernels' chains hold at most " + std::to_string(WBC_MAX_DEPTH) + " moving bodies)");
    if (!visited_.insert(link).second) return bad(kMalformed, "link " + link + " is reached twice (a loop, or two parent joints)");
    const Link& lk = links_[link_of_.at(link)];
    comp_[body] = merge(comp_[body], lk.mass, add(lk.com, offset), lk.inertia);
    auto it = children_.find(link);
    if (it == children_.end()) return 0;
    for (int ji : it->second) {   // children_ is not modified during the walk
      const Joint& j = joints_[ji];
      const std::string what = "joint " + j.name + at(j.line);
      for (int i = 0; i < 3; ++i)
        if (!(std::fabs(j.rpy[i]) <= 1e-8))
          return bad(kUnsupported, what + ": non-zero rpy; the kernels take unrotated joint frames");
      Vec3 off = add(offset, j.xyz);
      int rc;
      if (j.type == "fixed") {
        if (j.dont_collapse) add_rb(j.child, body, off);
        if ((rc = visit(j.child, body, off, depth + 1))) return rc;
      } else if (j.type == "prismatic" && j.friction >= o_.lock_friction_above) {
        // a DoF in the simulator's tensors, rigid in the dynamics (the fingers)
        dof_joint_.push_back(ji);
        dof_locked_.push_back(true);
        add_rb(j.child, body, off);
        if ((rc = visit(j.child, body, off, depth + 1))) return rc;
      } else if (j.type == "prismatic") {
        // a free slider would be a moving body of its own, and the kernels' moving bodies are all revolute (urdf_model refuses it too)
        return bad(kUnsupported, what + ": prismatic joint with friction " + std::to_string(j.friction) + " < lock_friction_above " +
                                 std::to_string(o_.lock_friction_above) + " is not locked; a sliding joint is not among the kernels' moving bodies "
                                 "(revolute only)");
      } else if (j.type == "revolute") {
        int ax = 0;   // np.argmax(|axis|), then np.allclose(|axis|, e_ax) and axis[ax] > 0
        for (int i = 1; i < 3; ++i)
          if (std::fabs(j.axis[i]) > std::fabs(j.axis[ax])) ax = i;
        bool ok = j.axis[ax] > 0;
        for (int i = 0; i < 3; ++i) {
          double e = i == ax ? 1.0 : 0.0;
          ok = ok && std::fabs(std::fabs(j.axis[i]) - e) <= 1e-8 + 1e-5 * e;
        }
        if (!ok) return bad(kUnsupported, what + ": axis must be +x, +y or +z");
        int nb_new = (int)parent_.size();
        parent_.push_back(body);
        axis_.push_back(ax);
        joint_xyz_.push_back(off);
        comp_.push_back(Body());
        body_dof_.push_back((int)dof_joint_.size());
        dof_joint_.push_back(ji);
        dof_locked_.push_back(false);
        add_rb(j.child, nb_new, Vec3{});
        if ((rc = visit(j.child, nb_new, Vec3{}, depth + 1))) return rc;
      } else {
        return bad(kUnsupported, what + ": type '" + j.type + "' is not supported (revolute, fixed, or prismatic locked by its friction)");
      }
    }
    return 0;
  }

  // build_model.collapsed_piece: a link and everything collapsed into it, in the Python stack's order
  Body collapsed_piece(const std::string& start, const Vec3& off0) {
    Body b;
    std::vector<std::pair<std::string, Vec3>> stack{{start, off0}};
    while (!stack.empty()) {
      std::pair<std::string, Vec3> top = stack.back();
      stack.pop_back();
      const Link& lk = links_[link_of_.at(top.first)];
      b = merge(b, lk.mass, add(lk.com, top.second), lk.inertia);
      auto it = children_.find(top.first);
      if (it == children_.end()) continue;
      for (int ji : it->second) {
        const Joint& j = joints_[ji];
        if (j.type == "fixed" && !j.dont_collapse) stack.push_back({j.child, add(top.second, j.xyz)});
      }
    }
    return b;
  }

  int build() {
    const std::string root = o_.root_link;
    if (!link_of_.count(root)) return bad(kUnsupported, "root_link '" + root + "' is not a link of the URDF");
    parent_.push_back(-1);
    axis_.push_back(-1);
    joint_xyz_.push_back(Vec3{});
    comp_.push_back(Body());
    body_dof_.push_back(-1);
    add_rb(root, 0, Vec3{});
    int rc = visit(root, 0, Vec3{}, 0);
    if (rc) return rc;
    int nb = (int)parent_.size(), ndof = (int)dof_joint_.size(), nrb = (int)rb_names_.size();
    if (nb != WBC_NB || ndof != WBC_NDOF || nrb != WBC_NRB)
      return bad(kUnsupported, "robot " + root + ": " + std::to_string(nb) + " moving bodies, " + std::to_string(ndof) + " DoFs, " + std::to_string(nrb) +
                               " rigid bodies; the kernels are compiled for " + std::to_string(WBC_NB) + " / " + std::to_string(WBC_NDOF) + " / " +
                               std::to_string(WBC_NRB));
    base_piece_ = collapsed_piece(root, Vec3{});
    base_rest_ = unmerge(comp_[0], base_piece_);
    int gi = rb_find(o_.gripper_name);
    if (gi < 0) return bad(kUnsupported, std::string("gripper_name '") + o_.gripper_name + "' is not a rigid body of the URDF");
    grip_body_ = rb_body_[gi];
    grip_piece_ = collapsed_piece(o_.gripper_name, rb_offset_[gi]);
    grip_rest_ = unmerge(comp_[grip_body_], grip_piece_);
    for (int ji : dof_joint_) out_.dof_names.push_back(joints_[ji].name);
    out_.rb_names = rb_names_;
    return 0;
  }

  int rb_find(const std::string& n) const {
    for (int i = 0; i < (int)rb_names_.size(); ++i)
      if (rb_names_[i] == n) return i;
    return -1;
  }

  // ---- abi.collision_set + quantise_reach + fill_model ------------------------------------------------------------------------
  struct Cp {
    int body = 0; Vec3 pos{}; double radius = 0.0; int rb = 0, kind = WBC_CP_TERRAIN, body2 = -1, rb2 = -1;
    Vec3 a{}, b{}; double radius2 = 0.0; int slot = 0, sph = -1;
  };
  struct Limb { std::string name; int s0, s1; double radius, cap0, cap1, length; int body, rb, rb0, rb1; };
  struct Cand { int kind, a, b; double reach; std::string what; };

  int quantise(double r, const std::string& what, float* out) {   // abi.quantise_reach: 3 bits of 0.04 m, rounded up
    const double step = 0.04;
    double code = std::ceil(r / step - 1e-9);
    if (!(code >= 1 && code <= 8))
      return bad(kUnsupported, what + ": bounding reach " + std::to_string(r) + " m does not fit the pair descriptor's 3 bits (0.04 .. 0.32 m)");
    *out = (float)(code * step);
    return 0;
  }

  int fill() {
    WBC_URDF_NO_FMA_CONTRACTION
    // abi.py's primitives of the URDF's <collision> blocks
    const Vec3 trunk_half{{0.3762 / 2, 0.0935 / 2, 0.114 / 2}};
    const double thigh_len = 0.213, thigh_radius = 0.017, corner_radius = 0.01, calf_len = 0.213, calf_radius = 0.008, box_corner_radius = 0.005;
    const double box_density = 1000.0, box_friction = 1.0, box_sleep_speed = 0.01, box_sleep_time = 0.4;
    const double knee_radius = 0.02, foot_radius = 0.02, elbow_radius = 0.025, wrist_radius = 0.025, grip_radius = 0.012;
    const double upper_arm_len = std::hypot(0.25, 0.04975), forearm_len = 0.25, hand_len = 0.1586;
    const double limb_rsum_max = 0.060;   // WBC_LIMB_RSUM_MAX, compared in double as abi.collision_set does
    const int static_self_slot0 = 23, box_row = 32, shank0 = 48, shoulder_slot = 26;
    static const char* const kLegs[4] = {"FL", "FR", "RL", "RR"};
    const bool self_coll = o_.self_collisions == 0;
    const double box_half = 0.5 * o_.box_size, rest = o_.rest_offset;

    wbc_model& M = out_.model;
    memset(&M, 0, sizeof(M));
    for (int i = 0; i < WBC_NB; ++i) {
      M.parent[i] = parent_[i];
      M.axis[i] = axis_[i];
      M.dof[i] = body_dof_[i];
      put3(M.joint_xyz[i], joint_xyz_[i]);
      M.mass[i] = (float)comp_[i].m;
      put3(M.com[i], comp_[i].c);
      sym6(comp_[i].I, M.inertia[i]);
    }
    for (int i = 0; i < WBC_NDOF; ++i) {
      const Joint& j = joints_[dof_joint_[i]];
      M.q_lower[i] = (float)j.lower;
      M.q_upper[i] = (float)j.upper;
      M.qd_limit[i] = (float)j.velocity;
      M.effort[i] = (float)j.effort;
      out_.lower.push_back(j.lower);
      out_.upper.push_back(j.upper);
      out_.velocity.push_back(j.velocity);
      out_.effort.push_back(j.effort);
      wbc_dof_props p;
      memset(&p, 0, sizeof(p));
      p.has_limits = !(j.lower == 0.0 && j.upper == 0.0);
      p.lower = (float)j.lower;
      p.upper = (float)j.upper;
      p.drive_mode = o_.default_dof_drive_mode;
      p.velocity = (float)j.velocity;
      p.effort = (float)j.effort;
      p.damping = (float)j.damping;
      p.friction = (float)j.friction;
      p.armature = (float)o_.armature;
      p.locked = dof_locked_[i] ? 1 : 0;
      out_.props.push_back(p);
    }
    for (int i = 0; i < WBC_NRB; ++i) {
      M.rb_body[i] = rb_body_[i];
      put3(M.rb_offset[i], rb_offset_[i]);
    }
    const auto& rbn = rb_names_;
    std::vector<int> feet;   // WG:297
    for (int i = 0; i < WBC_NRB; ++i)
      if (rbn[i].find(o_.foot_name) != std::string::npos) feet.push_back(i);
    if ((int)feet.size() != WBC_NFEET)
      return bad(kUnsupported, std::string("foot_name '") + o_.foot_name + "' matches " + std::to_string(feet.size()) + " rigid bodies, not " +
                               std::to_string(WBC_NFEET));
    for (int i = 0; i < WBC_NFEET; ++i) {
      int rb = feet[i];
      if (rb < 2 || rbn[rb - 1].find("calf") == std::string::npos || rbn[rb - 2].find("thigh") == std::string::npos)
        return bad(kUnsupported, "foot " + rbn[rb] + ": the two rigid bodies before it must be its calf and its thigh");
      if (self_coll && rbn[rb].compare(0, 2, kLegs[i]) != 0)
        return bad(kUnsupported, "foot " + rbn[rb] + ": the feet must come in the order FL, FR, RL, RR");
      M.feet_rb[i] = rb;
    }
    M.gripper_rb = rb_find(o_.gripper_name);
    std::vector<std::string> need{"trunk", "wx250s/upper_arm_link", "wx250s/upper_forearm_link", "wx250s/wrist_link"};
    if (self_coll) need.push_back("wx250s/gripper_link");
    for (const auto& n : need)
      if (rb_find(n) < 0) return bad(kUnsupported, "rigid body " + n + " (a collision primitive rides on it) is not in the URDF");
    const int trunk_rb = rb_find("trunk");

    std::vector<Cp> cps;
    auto sphere = [&](int rb, const Vec3& pos, double rad, int slot = -1, int sph = -1) {
      Cp c;
      c.body = rb_body_[rb];
      c.pos = add(rb_offset_[rb], pos);
      c.radius = rad;
      c.rb = rb;
      c.slot = slot < 0 ? (int)cps.size() : slot;
      c.sph = sph < 0 ? (int)cps.size() : sph;
      cps.push_back(c);
      return (int)cps.size() - 1;
    };
    for (int rb : feet) sphere(rb, Vec3{}, foot_radius);
    for (int rb : feet) sphere(rb - 1, Vec3{}, knee_radius);   // knees = calf origins
    const int k_grip = sphere(M.gripper_rb, Vec3{}, grip_radius);
    const int k_elbow = sphere(rb_find("wx250s/upper_forearm_link"), Vec3{}, elbow_radius);
    const int k_wrist = sphere(rb_find("wx250s/wrist_link"), Vec3{}, wrist_radius);
    for (int rb : feet) sphere(rb - 2, Vec3{}, thigh_radius);
    const double hx = trunk_half[0] - corner_radius, hy = trunk_half[1] - corner_radius, hz = trunk_half[2] - corner_radius;
    for (int sx : {1, -1})
      for (int sy : {1, -1})
        for (int sz : {-1, 1}) sphere(trunk_rb, Vec3{{sx * hx, sy * hy, sz * hz}}, corner_radius);
    for (int i = 0; i < 4; ++i) sphere(feet[i] - 1, Vec3{{0.0, 0.0, -calf_len / 2}}, calf_radius, shank0 + i, static_self_slot0 + i);
    const int k_shoulder = sphere(rb_find("wx250s/upper_arm_link"), Vec3{}, elbow_radius, shoulder_slot, WBC_NSPH - 1);
    const double hb = box_half - box_corner_radius;   // the free box: corner spheres inset so that the surface is the cube's
    int hi = box_row;
    for (int sx : {1, -1})
      for (int sy : {1, -1})
        for (int sz : {-1, 1}) {
          Cp c;
          c.body = WBC_BOX_BODY;
          c.pos = Vec3{{sx * hb, sy * hb, sz * hb}};
          c.radius = box_corner_radius;
          c.rb = WBC_BOX_RB;
          c.slot = hi++;
          c.sph = -1;
          cps.push_back(c);
        }
    std::vector<Limb> limbs;
    std::vector<Cand> cands;
    if (self_coll) {
      int lo = static_self_slot0;
      auto pair = [&](int k, int body2, int rb2, const Vec3& a, const Vec3& b, int slot) {
        Cp c = cps[k];
        c.kind = WBC_CP_BOX; c.body2 = body2; c.rb2 = rb2; c.a = a; c.b = b; c.radius2 = 0.0; c.slot = slot;
        cps.push_back(c);
      };
      for (int k : {k_grip, k_wrist, k_elbow}) pair(k, rb_body_[trunk_rb], trunk_rb, rb_offset_[trunk_rb], trunk_half, lo++);
      for (int k : {0, 1, 2, 3, k_grip}) pair(k, WBC_BOX_BODY, WBC_BOX_RB, Vec3{}, Vec3{{box_half, box_half, box_half}}, hi++);
      std::vector<int> dyn;
      for (int s = 27; s < 32; ++s) dyn.push_back(s);
      for (int s = 52; s < 64; ++s) dyn.push_back(s);
      for (int s : {45, 46, 47}) dyn.push_back(s);
      for (int s : dyn) {
        Cp c;
        c.kind = WBC_CP_DYNAMIC;
        c.slot = s;
        cps.push_back(c);
      }
      for (int i = 0; i < 4; ++i)
        limbs.push_back(Limb{std::string(kLegs[i]) + "_thigh", 11 + i, 4 + i, thigh_radius, 0.0, 0.0, thigh_len, rb_body_[feet[i] - 2], feet[i] - 2,
                             feet[i] - 2, feet[i] - 2});
      for (int i = 0; i < 4; ++i)
        limbs.push_back(Limb{std::string(kLegs[i]) + "_calf", 4 + i, i, calf_radius, knee_radius, foot_radius, calf_len, rb_body_[feet[i] - 1],
                             feet[i] - 1, feet[i] - 1, feet[i]});
      const auto& fit = o_.arm_limb_fit;
      const int grip_link = rb_find("wx250s/gripper_link");
      limbs.push_back(Limb{"upper_arm", WBC_NSPH - 1, k_elbow, fit[0][0], fit[0][1], fit[0][2], upper_arm_len, cps[k_shoulder].body, cps[k_shoulder].rb,
                           cps[k_shoulder].rb, cps[k_shoulder].rb});
      limbs.push_back(Limb{"forearm", k_elbow, k_wrist, fit[1][0], fit[1][1], fit[1][2], forearm_len, cps[k_elbow].body, cps[k_elbow].rb,
                           cps[k_elbow].rb, cps[k_wrist].rb});
      limbs.push_back(Limb{"hand", k_wrist, k_grip, fit[2][0], fit[2][1], fit[2][2], hand_len, cps[k_grip].body, grip_link, grip_link, grip_link});
      auto L = [&](const std::string& n) {
        for (int i = 0; i < (int)limbs.size(); ++i)
          if (limbs[i].name == n) return i;
        return -1;
      };
      auto maxr = [](const Limb& l) { return std::max(l.radius, std::max(l.cap0, l.cap1)); };
      auto bound = [&](const Limb& l) { return 0.5 * l.length + maxr(l); };
      auto limb_pair = [&](const std::string& a, const std::string& b) {
        int ia = L(a), ib = L(b);
        cands.push_back(Cand{WBC_PR_LIMBS, ia, ib, bound(limbs[ia]) + bound(limbs[ib]), "limb pair " + a + " / " + b});
      };
      const std::pair<const char*, const char*> side[2] = {{"FL", "RL"}, {"FR", "RR"}}, lr[2] = {{"FL", "FR"}, {"RL", "RR"}},
                                                diag[2] = {{"FL", "RR"}, {"FR", "RL"}};
      std::vector<std::pair<const char*, const char*>> side_lr{side[0], side[1], lr[0], lr[1]};
      for (const auto& ab : side_lr) limb_pair(std::string(ab.first) + "_calf", std::string(ab.second) + "_calf");
      for (const auto& ab : side_lr) {
        limb_pair(std::string(ab.first) + "_calf", std::string(ab.second) + "_thigh");
        limb_pair(std::string(ab.second) + "_calf", std::string(ab.first) + "_thigh");
      }
      for (const auto& ab : lr) limb_pair(std::string(ab.first) + "_thigh", std::string(ab.second) + "_thigh");
      for (const char* arm : {"upper_arm", "forearm", "hand"})
        for (const char* leg : kLegs)
          for (const char* part : {"_thigh", "_calf"}) limb_pair(arm, std::string(leg) + part);
      for (const auto& ab : diag) {
        limb_pair(std::string(ab.first) + "_calf", std::string(ab.second) + "_calf");
        limb_pair(std::string(ab.first) + "_calf", std::string(ab.second) + "_thigh");
        limb_pair(std::string(ab.second) + "_calf", std::string(ab.first) + "_thigh");
      }
      for (const Cand& c : cands)
        if (!(maxr(limbs[c.a]) + maxr(limbs[c.b]) <= limb_rsum_max))
          return bad(kUnsupported, c.what + ": radius sum " + std::to_string(maxr(limbs[c.a]) + maxr(limbs[c.b])) +
                                   " m exceeds WBC_LIMB_RSUM_MAX (0.060 m); check arm_limb_fit");
      // robot spheres that can meet the free box besides the five static pairs: knees, shins, the trunk box's bottom corners
      std::vector<int> spheres{4, 5, 6, 7};
      for (int i = 0; i < 4; ++i) spheres.push_back(static_self_slot0 + i);
      for (int k = 15; k < 23; ++k)
        if (cps[k].pos[2] < rb_offset_[trunk_rb][2]) spheres.push_back(k);
      for (int k : spheres) {
        double rad = 0.0;
        for (const Cp& c : cps)
          if (c.sph == k && c.kind == WBC_CP_TERRAIN) { rad = c.radius; break; }
        cands.push_back(Cand{WBC_PR_SPHERE_BOX, k, 0, box_half * std::sqrt(3.0) + rad, "robot sphere " + std::to_string(k) + " / free box"});
      }
      if (cands.size() != 56)
        return bad(kUnsupported, "trunk: " + std::to_string(cands.size() - 44) + " robot spheres can meet the free box, the collision set has 12");
    }
    std::stable_sort(cps.begin(), cps.end(), [](const Cp& a, const Cp& b) { return a.slot < b.slot; });

    M.box_half = (float)box_half;
    M.box_mass = (float)(box_density * std::pow(o_.box_size, 3.0));
    M.box_friction = (float)box_friction;
    M.box_sleep_speed = (float)box_sleep_speed;
    M.box_sleep_time = (float)box_sleep_time;
    int ncp = 0;
    for (const Cp& c : cps) ncp = std::max(ncp, c.slot + 1);
    M.ncp = ncp;
    for (int k = 0; k < WBC_NCP; ++k) {
      M.cp_body2[k] = M.cp_rb2[k] = M.cp_sph[k] = -1;
      M.cp_kind[k] = WBC_CP_NONE;
      M.pr_kind[k] = WBC_PR_NONE;
    }
    for (const Cp& c : cps) {
      int k = c.slot;
      M.cp_body[k] = c.body; M.cp_rb[k] = c.rb; M.cp_kind[k] = c.kind;
      M.cp_body2[k] = c.body2; M.cp_rb2[k] = c.rb2;
      M.cp_radius[k] = (float)(c.radius + (c.kind != WBC_CP_DYNAMIC ? rest : 0.0));
      M.cp_radius2[k] = (float)c.radius2;
      M.cp_sph[k] = c.sph;
      put3(M.cp_pos[k], c.pos);
      put3(M.cp_a[k], c.a);
      put3(M.cp_b[k], c.b);
      if (c.kind == WBC_CP_BOX) {   // the lane's own pair is what it tests in the broad phase
        M.pr_kind[k] = WBC_PR_STATIC; M.pr_a[k] = c.sph; M.pr_b[k] = 0;
        int rc = quantise(std::sqrt(dot3(c.b, c.b)) + (double)M.cp_radius[k], "static pair in slot " + std::to_string(k), &M.pr_reach[k]);
        if (rc) return rc;
      }
    }
    M.nlimb = (int)limbs.size();
    for (int i = 0; i < (int)limbs.size(); ++i) {
      const Limb& l = limbs[i];
      M.limb_s0[i] = l.s0; M.limb_s1[i] = l.s1;
      M.limb_radius[i] = (float)l.radius; M.limb_cap0[i] = (float)l.cap0; M.limb_cap1[i] = (float)l.cap1;
      M.limb_body[i] = l.body; M.limb_rb[i] = l.rb; M.limb_rb0[i] = l.rb0; M.limb_rb1[i] = l.rb1;
    }
    M.pair_rest_offset = (float)rest;
    size_t ci = 0;   // every lane without a static pair of its own tests a candidate
    for (int k = 0; k < WBC_NCP && ci < cands.size(); ++k) {
      if (M.pr_kind[k] == WBC_PR_STATIC) continue;
      const Cand& c = cands[ci++];
      M.pr_kind[k] = c.kind; M.pr_a[k] = c.a; M.pr_b[k] = c.b;
      int rc = quantise(c.reach + rest, c.what, &M.pr_reach[k]);
      if (rc) return rc;
    }
    M.base_piece_mass = (float)base_piece_.m;
    put3(M.base_piece_com, base_piece_.c);
    sym6(base_piece_.I, M.base_piece_inertia);
    M.base_rest_mass = (float)base_rest_.m;
    put3(M.base_rest_com, base_rest_.c);
    sym6(base_rest_.I, M.base_rest_inertia);
    M.gripper_body = grip_body_;
    M.grip_piece_mass = (float)grip_piece_.m;
    put3(M.grip_piece_com, grip_piece_.c);
    sym6(grip_piece_.I, M.grip_piece_inertia);
    M.grip_rest_mass = (float)grip_rest_.m;
    put3(M.grip_rest_com, grip_rest_.c);
    sym6(grip_rest_.I, M.grip_rest_inertia);
    return 0;
  }
};

// Reads and builds; 0, or -2 / -4 with `err` naming the file's element. `out` is complete only on 0.
inline int load(const char* path, const wbc_asset_opts& o, Result& out, std::string& err) {
  int rc = check_opts(o, err);
  if (rc) return rc;
  FILE* f = fopen(path, "rb");
  if (!f) { err = std::string("cannot open ") + path; return kMalformed; }
  std::string text;
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, n);
  bool read_error = ferror(f) != 0;
  fclose(f);
  if (read_error) { err = std::string("cannot read ") + path; return kMalformed; }
  rc = Loader(o, out, err).run(text);
  if (rc) err = std::string(path) + ": " + err;
  return rc;
}

// abi.set_soft_limits (LR:294-304) and fill_task_cfg's torque_limits (LR:294-299) from the URDF's limits
inline void set_model_limits(wbc_task_cfg& cfg, const Result& r, const wbc_asset_opts& o) {
  WBC_URDF_NO_FMA_CONTRACTION
  for (int i = 0; i < WBC_NDOF; ++i) {
    double lo = r.lower[i], hi = r.upper[i];
    double mid = 0.5 * (lo + hi), rng = hi - lo;
    cfg.torque_limits[i] = (float)r.effort[i];
    cfg.soft_dof_lower[i] = (float)(mid - 0.5 * rng * o.soft_dof_pos_limit);
    cfg.soft_dof_upper[i] = (float)(mid + 0.5 * rng * o.soft_dof_pos_limit);
    cfg.soft_dof_vel_limit[i] = (float)(r.velocity[i] * o.soft_dof_vel_limit);
    cfg.soft_torque_limit[i] = (float)(r.effort[i] * o.soft_torque_limit);
  }
}

}  // namespace wbc_urdf
