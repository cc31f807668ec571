// Scene ingestion for the HIP core without Python: Hydra XML scene description + VSGF meshes + image4ub
// textures + IES photometry -> the flat tables hpt_upload_scene / hpt_add_geom_triangles3f / hpt_add_instance / hpt_update_params take.
//
// Follows the reference's loaders for the material / light subset of the hot path:
//   LoadScene / LoadSceneGeometry / LoadSceneInstances / LoadSceneSettings   integrator_pt_scene.cpp:645-1076
//   ConvertOldHydraMaterial (every branch: diffuse, Oren-Nayar, metal mix, coated plastic, metal, glass, emission)   integrator_pt_scene_mat.cpp:280-450
//   LoadLightSourceFromNode (rect, disk, sphere, point / spot / IES, directional, plain-colour sky)   integrator_pt_scene_lgt.cpp:5-222
//   LoadTextureAndMakeCombined / image4ub                                       integrator_pt_scene_tex.cpp:7-144
//   cmesh4::LoadMeshFromVSGF                                                    external/LiteScene/cmesh4.cpp:140-167
//   CreateSphericalTextureFromIES (axially symmetric photometry)               ies_parser/ies_render.cpp:29-120
// and produces the same tables as the Python fixture loader (hydracore3_amd/scene.py; tests compare the two byte for byte, matrices
// to float rounding). Header-only host C++17, no dependencies: the XML subset Hydra writes (elements, attributes, text, comments)
// is parsed by the ~80 lines below instead of pugixml.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <array>
#include <map>
#include <unordered_map>
#include <sstream>
#include <string>
#include <vector>

#include <zlib.h>                       // inflate for PNG textures (link the tools with -lz)
#include "integrator_hip.h"
#include "plastic_precompute.h"
#include "film_precompute.h"
#include "jpeg_decode.h"
#include "cie_fit.h"
#include <set>

namespace hydra_hip {

// ---- minimal XML --------------------------------------------------------------------------------------------------------------
struct XmlNode
{
  std::string name, text;
  std::map<std::string, std::string> attr;
  std::vector<XmlNode> children;
  const XmlNode* child(const std::string& n) const { for (const XmlNode& c : children) if (c.name == n) return &c; return nullptr; }
  std::vector<const XmlNode*> all(const std::string& n) const { std::vector<const XmlNode*> r; for (const XmlNode& c : children) if (c.name == n) r.push_back(&c); return r; }
  const XmlNode* path(const std::string& p) const
  {
    const XmlNode* cur = this; size_t a = 0;
    while (cur && a <= p.size()) { const size_t b = p.find('/', a); cur = cur->child(p.substr(a, b == std::string::npos ? std::string::npos : b - a)); if (b == std::string::npos) break; a = b + 1; }
    return cur;
  }
  bool has(const std::string& k) const { return attr.count(k) != 0; }
  std::string get(const std::string& k, const std::string& dflt = "") const { auto it = attr.find(k); return it == attr.end() ? dflt : it->second; }
  std::string childText(const std::string& n) const { const XmlNode* c = child(n); return c ? c->text : std::string(); }
};

class XmlParser
{
public:
  explicit XmlParser(const std::string& s) : t(s) {}
  bool parse(XmlNode& root, std::string& err)
  {
    root.name = "root";
    while (true) {
      skipMisc();
      if (i >= t.size()) return true;
      if (t[i] != '<') { err = "xml: text outside of an element"; return false; }
      XmlNode n; if (!element(n, err)) return false;
      root.children.push_back(std::move(n));
    }
  }
private:
  const std::string& t; size_t i = 0;
  void ws() { while (i < t.size() && std::isspace((unsigned char)t[i])) i++; }
  void skipMisc()
  {
    while (true) {
      ws();
      if (t.compare(i, 4, "<!--") == 0) { const size_t e = t.find("-->", i); i = e == std::string::npos ? t.size() : e + 3; }
      else if (t.compare(i, 2, "<?") == 0) { const size_t e = t.find("?>", i); i = e == std::string::npos ? t.size() : e + 2; }
      else return;
    }
  }
  static std::string trim(const std::string& s)
  {
    size_t a = 0, b = s.size();
    while (a < b && std::isspace((unsigned char)s[a])) a++;
    while (b > a && std::isspace((unsigned char)s[b - 1])) b--;
    return s.substr(a, b - a);
  }
  bool element(XmlNode& n, std::string& err)
  {
    i++;                                                    // '<'
    const size_t a = i;
    while (i < t.size() && !std::isspace((unsigned char)t[i]) && t[i] != '>' && t[i] != '/') i++;
    n.name = t.substr(a, i - a);
    while (true) {                                          // attributes
      ws();
      if (i >= t.size()) { err = "xml: unterminated tag <" + n.name; return false; }
      if (t[i] == '/') { i += 2; return true; }             // "/>"
      if (t[i] == '>') { i++; break; }
      const size_t k0 = i;
      while (i < t.size() && t[i] != '=' && !std::isspace((unsigned char)t[i])) i++;
      const std::string key = t.substr(k0, i - k0);
      ws(); if (i >= t.size() || t[i] != '=') { err = "xml: attribute without value in <" + n.name; return false; }
      i++; ws();
      const char q = t[i]; if (q != '"' && q != '\'') { err = "xml: unquoted attribute in <" + n.name; return false; }
      const size_t v0 = ++i; const size_t v1 = t.find(q, v0);
      if (v1 == std::string::npos) { err = "xml: unterminated attribute in <" + n.name; return false; }
      n.attr[key] = t.substr(v0, v1 - v0); i = v1 + 1;
    }
    std::string text;
    while (true) {                                          // content
      const size_t lt = t.find('<', i);
      if (lt == std::string::npos) { err = "xml: missing </" + n.name + ">"; return false; }
      text += t.substr(i, lt - i); i = lt;
      if (t.compare(i, 4, "<!--") == 0) { const size_t e = t.find("-->", i); i = e == std::string::npos ? t.size() : e + 3; continue; }
      if (t.compare(i, 2, "</") == 0) { const size_t e = t.find('>', i); i = e == std::string::npos ? t.size() : e + 1; break; }
      XmlNode c; if (!element(c, err)) return false;
      n.children.push_back(std::move(c));
    }
    n.text = trim(text);
    return true;
  }
};

// ---- small double-precision matrix helpers (row-major [r][c]; the tables store LiteMath's column-major float) ---------------------
struct M4 { double m[4][4]; };
inline M4 m4Identity() { M4 r; for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) r.m[a][b] = a == b ? 1.0 : 0.0; return r; }
inline M4 m4Mul(const M4& A, const M4& B) { M4 r; for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) { double s = 0; for (int k = 0; k < 4; k++) s += A.m[a][k] * B.m[k][b]; r.m[a][b] = s; } return r; }
inline M4 m4Transpose(const M4& A) { M4 r; for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) r.m[a][b] = A.m[b][a]; return r; }
inline M4 m4Inverse(const M4& A)                             // Gauss-Jordan with partial pivoting
{
  double a[4][8];
  for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) { a[r][c] = A.m[r][c]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
  for (int c = 0; c < 4; c++) {
    int p = c; for (int r = c + 1; r < 4; r++) if (std::fabs(a[r][c]) > std::fabs(a[p][c])) p = r;
    if (p != c) for (int k = 0; k < 8; k++) std::swap(a[p][k], a[c][k]);
    const double d = a[c][c];
    for (int k = 0; k < 8; k++) a[c][k] /= d;
    for (int r = 0; r < 4; r++) if (r != c) { const double f = a[r][c]; if (f != 0.0) for (int k = 0; k < 8; k++) a[r][k] -= f * a[c][k]; }
  }
  M4 R; for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) R.m[r][c] = a[r][4 + c];
  return R;
}
inline void m4ToColMajor(const M4& A, float out[16]) { for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) out[c * 4 + r] = (float)A.m[r][c]; }
inline std::vector<double> parseFloats(const std::string& s) { std::vector<double> v; std::istringstream is(s); double x; while (is >> x) v.push_back(x); return v; }
// LiteMath::perspectiveMatrix / lookAt (OpenGL conventions), in double
inline M4 m4Perspective(double fovDeg, double aspect, double zNear, double zFar)
{
  const double ymax = zNear * std::tan(fovDeg * M_PI / 360.0), xmax = ymax * aspect;
  const double left = -xmax, right = xmax, bottom = -ymax, top = ymax;
  const double t = 2.0 * zNear, t2 = right - left, t3 = top - bottom, t4 = zFar - zNear;
  M4 proj; std::memset(&proj, 0, sizeof(proj));
  proj.m[0][0] = t / t2; proj.m[1][1] = t / t3; proj.m[0][2] = (right + left) / t2; proj.m[1][2] = (top + bottom) / t3;
  proj.m[2][2] = (-zFar - zNear) / t4; proj.m[3][2] = -1.0; proj.m[2][3] = (-t * zFar) / t4;
  return proj;
}
inline M4 m4LookAt(const double* eye, const double* center, const double* up)
{
  double f[3] = { center[0] - eye[0], center[1] - eye[1], center[2] - eye[2] };
  const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]); for (double& x : f) x /= fl;
  const double ul = std::sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
  const double un[3] = { up[0] / ul, up[1] / ul, up[2] / ul };
  double s[3] = { f[1] * un[2] - f[2] * un[1], f[2] * un[0] - f[0] * un[2], f[0] * un[1] - f[1] * un[0] };
  const double sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]); for (double& x : s) x /= sl;
  const double u[3] = { s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0] };
  M4 wv = m4Identity();
  for (int k = 0; k < 3; k++) { wv.m[0][k] = s[k]; wv.m[1][k] = u[k]; wv.m[2][k] = -f[k]; }
  wv.m[0][3] = -(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2]);
  wv.m[1][3] = -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]);
  wv.m[2][3] = (f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2]);
  return wv;
}
inline M4 m4FromText(const std::string& s) { M4 r = m4Identity(); const std::vector<double> v = parseFloats(s); for (int k = 0; k < 16 && k < (int)v.size(); k++) r.m[k / 4][k % 4] = v[k]; return r; }

// ---- the loaded scene --------------------------------------------------------------------------------------------------------------
struct LoadedTexture { uint32_t width = 1, height = 1, format = 0, flags = 0, addressU = 0, addressV = 0, filter = 1; std::vector<uint8_t> bytes; };

struct LoadedScene
{
  std::vector<float> vPos4f, vData8f, instMatrices, normMatrices;
  // motion blur (integrator_pt_scene.cpp:848-897): <motion matrix=..> of an instance; once one moves, normMatrices gets a second half
  std::vector<float> instMatricesMotion; std::vector<uint32_t> instHasMotion; uint32_t normMatrices2Offs = 0;
  std::vector<uint32_t> triIndices, matIdByPrimId, matVertOffset, geomTriCount, geomVertCount, instGeomId;
  std::vector<int32_t> remapInst, allRemapLists{0};
  uint32_t allRemapListsSize = 0;
  std::vector<Material> materials;
  std::vector<LightSource> lights;
  std::vector<LoadedTexture> textures;
  int width = 512, height = 512;
  double fov = 45.0, nearClip = 0.01, farClip = 100.0, camPos[3] = {0, 0, 15}, camLookAt[3] = {0, 0, 0}, camUp[3] = {0, 1, 0};
  uint32_t traceDepth = 6, spp = 1;
  float envColor[4] = {0, 0, 0, 0};
  // the environment map of LoadSceneLights (integrator_pt_scene.cpp:441-478) and m_arrays1f (its pdf table)
  uint32_t envTexId = 0xFFFFFFFFu, envLightId = 0xFFFFFFFFu, envCamBackId = 0xFFFFFFFFu, envEnableSam = 0;
  float envSamRow0[4] = {1, 0, 0, 0}, envSamRow1[4] = {0, 1, 0, 0};
  uint32_t envSpecId = 0xFFFFFFFFu; float envSpecMult = 1.0f;   // m_envSpecId, m_envSpecMult (integrator_pt_scene.cpp:456-457)
  std::vector<float> arrays1f;
  // thin films (integrator_pt.h:587-590): m_films_thickness_vec, m_films_spec_id_vec, m_films_eta_k_vec, m_precomp_thin_films
  std::vector<float> filmsThickness, filmsEtaK, precompThinFilms; std::vector<uint32_t> filmsSpecId;
  std::vector<uint32_t> specTexIdsWavelengths, specTexOffsetSz;   // spectra given by textures: uint2 {texture, wavelength} per band, uint2 {first band, bands} per spectrum
  std::vector<float> lensLines; float physSize[2] = {0, 0};   // lens simulation: m_lines as {curvatureRadius, thickness, eta, apertureRadius}, m_physSize
  // spectral rendering (LoadSceneSpectrumData, integrator_pt_scene.cpp:358-419; the camera's <sensor><response>, :688-711)
  uint32_t spectralMode = 0;
  std::vector<float> specValues; std::vector<uint32_t> specOffsetSz; std::vector<float> cieXYZ;
  int32_t camResponseSpectrumId[3] = {-1, -1, -1}; uint32_t camResponseType = 0; float camRespoceRGB[4] = {1, 1, 1, 1};
  std::vector<hpt_texture_desc> texDescs;                 // filled by desc(): points into `textures`

  hpt_scene_desc desc()
  {
    hpt_scene_desc d; std::memset(&d, 0, sizeof(d));
    d.numGeoms = (uint32_t)geomTriCount.size(); d.numInsts = (uint32_t)instGeomId.size();
    d.numVerts = (uint32_t)(vPos4f.size() / 4); d.numTris = (uint32_t)matIdByPrimId.size();
    d.vPos4f = vPos4f.data(); d.vData8f = vData8f.data(); d.triIndices = triIndices.data(); d.matIdByPrimId = matIdByPrimId.data();
    d.matVertOffset = matVertOffset.data(); d.geomTriCount = geomTriCount.data(); d.geomVertCount = geomVertCount.data();
    d.instGeomId = instGeomId.data(); d.instMatrices = instMatrices.data(); d.normMatrices = normMatrices.data();
    d.remapInst = remapInst.data(); d.allRemapLists = allRemapLists.data();
    d.allRemapListsLen = (uint32_t)allRemapLists.size(); d.allRemapListsSize = allRemapListsSize;
    d.materials = materials.data(); d.numMaterials = (uint32_t)materials.size();
    d.lights = lights.empty() ? nullptr : lights.data(); d.numLights = (uint32_t)lights.size();
    texDescs.resize(textures.size());
    for (size_t i = 0; i < textures.size(); i++) {
      const LoadedTexture& t = textures[i]; hpt_texture_desc& o = texDescs[i]; std::memset(&o, 0, sizeof(o));
      o.width = t.width; o.height = t.height; o.format = t.format; o.flags = t.flags; o.addressU = t.addressU; o.addressV = t.addressV; o.filter = t.filter;
      o.data = t.bytes.data();
    }
    d.textures = texDescs.data(); d.numTextures = (uint32_t)texDescs.size();
    d.arrays1f = arrays1f.empty() ? nullptr : arrays1f.data(); d.numArrays1f = (uint32_t)arrays1f.size();
    if (normMatrices2Offs) { d.instMatricesMotion = instMatricesMotion.data(); d.instHasMotion = instHasMotion.data(); d.normMatrices2Offs = normMatrices2Offs; }
    for (int k = 0; k < 3; k++) d.camResponseSpectrumId[k] = -1;
    if (!specOffsetSz.empty()) {
      d.specValues = specValues.data(); d.numSpecValues = (uint32_t)specValues.size();
      d.specOffsetSz = specOffsetSz.data(); d.numSpectra = (uint32_t)(specOffsetSz.size() / 2);
      d.cieXYZ = cieXYZ.data(); d.numCieXYZ = (uint32_t)(cieXYZ.size() / 4);
      for (int k = 0; k < 3; k++) d.camResponseSpectrumId[k] = camResponseSpectrumId[k];
      d.camResponseType = camResponseType;
    }
    if (!specTexIdsWavelengths.empty() && specTexOffsetSz.size() == specOffsetSz.size()) {
      d.specTexIdsWavelengths = specTexIdsWavelengths.data(); d.numSpecTexBands = (uint32_t)(specTexIdsWavelengths.size() / 2); d.specTexOffsetSz = specTexOffsetSz.data();
    }
    if (!filmsEtaK.empty()) {
      d.filmsThickness = filmsThickness.data(); d.numFilmsThickness = (uint32_t)filmsThickness.size();
      d.filmsSpecId = filmsSpecId.data(); d.numFilmsSpecId = (uint32_t)filmsSpecId.size();
      d.filmsEtaK = filmsEtaK.data(); d.numFilmsEtaK = (uint32_t)filmsEtaK.size();
      d.precompThinFilms = precompThinFilms.empty() ? nullptr : precompThinFilms.data(); d.numPrecompThinFilms = (uint32_t)precompThinFilms.size();
    }
    return d;
  }

  uint32_t tileSize() const { for (uint32_t ts : {8u, 4u, 2u}) if (width % (int)ts == 0 && height % (int)ts == 0) return ts; return 1u; }   // SetViewport (integrator_pt.h:379-389)

  hpt_params params(uint32_t integratorType = 2, uint32_t renderLayer = 0) const
  {
    hpt_params p; std::memset(&p, 0, sizeof(p));
    // perspectiveMatrix / lookAt as LiteMath defines them (OpenGL conventions), inverted in double
    const double aspect = double(width) / double(height);
    const double ymax = nearClip * std::tan(fov * M_PI / 360.0), xmax = ymax * aspect;
    const double left = -xmax, right = xmax, bottom = -ymax, top = ymax;
    const double t = 2.0 * nearClip, t2 = right - left, t3 = top - bottom, t4 = farClip - nearClip;
    M4 proj; std::memset(&proj, 0, sizeof(proj));
    proj.m[0][0] = t / t2; proj.m[1][1] = t / t3; proj.m[0][2] = (right + left) / t2; proj.m[1][2] = (top + bottom) / t3;
    proj.m[2][2] = (-farClip - nearClip) / t4; proj.m[3][2] = -1.0; proj.m[2][3] = (-t * farClip) / t4;
    double f[3] = { camLookAt[0] - camPos[0], camLookAt[1] - camPos[1], camLookAt[2] - camPos[2] };
    const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]); for (double& x : f) x /= fl;
    const double ul = std::sqrt(camUp[0] * camUp[0] + camUp[1] * camUp[1] + camUp[2] * camUp[2]);
    const double un[3] = { camUp[0] / ul, camUp[1] / ul, camUp[2] / ul };
    double s[3] = { f[1] * un[2] - f[2] * un[1], f[2] * un[0] - f[0] * un[2], f[0] * un[1] - f[1] * un[0] };
    const double sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]); for (double& x : s) x /= sl;
    const double u[3] = { s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0] };
    M4 wv = m4Identity();
    for (int k = 0; k < 3; k++) { wv.m[0][k] = s[k]; wv.m[1][k] = u[k]; wv.m[2][k] = -f[k]; }
    wv.m[0][3] = -(s[0] * camPos[0] + s[1] * camPos[1] + s[2] * camPos[2]);
    wv.m[1][3] = -(u[0] * camPos[0] + u[1] * camPos[1] + u[2] * camPos[2]);
    wv.m[2][3] = (f[0] * camPos[0] + f[1] * camPos[1] + f[2] * camPos[2]);
    m4ToColMajor(m4Inverse(proj), p.projInv); m4ToColMajor(m4Inverse(wv), p.worldViewInv);
    p.winStartX = p.winStartY = 0; p.winWidth = p.fbWidth = width; p.winHeight = p.fbHeight = height;
    p.traceDepth = traceDepth; p.integratorType = integratorType; p.renderLayer = renderLayer; p.tileSize = tileSize(); p.spectralMode = spectralMode;
    p.envSpecIdPlus1 = envSpecId + 1u; p.envSpecMult = envSpecMult;
    p.exposureMult = 1.0f; p.camLensRadius = 0.0f; p.camTargetDist = (float)fl;
    for (int k = 0; k < 4; k++) { p.camRespoceRGB[k] = camRespoceRGB[k]; p.envColor[k] = envColor[k]; p.envSamRow0[k] = envSamRow0[k]; p.envSamRow1[k] = envSamRow1[k]; }
    p.envTexId = envTexId; p.envLightId = envLightId; p.envCamBackId = envCamBackId; p.envEnableSam = envEnableSam;
    return p;
  }

  // feed a context: geometry -> BVH, tables, parameters, pixel order, generators (what main.cpp:249-267 does through the Integrator)
  int upload(hpt_ctx* ctx, uint32_t integratorType = 2)
  {
    int rc = hpt_clear_geom(ctx); if (rc) return rc;
    for (size_t g = 0; g < geomTriCount.size(); g++) {
      const uint32_t triOff = matVertOffset[2 * g], vertOff = matVertOffset[2 * g + 1];
      if (hpt_add_geom_triangles3f(ctx, vPos4f.data() + 4 * (size_t)vertOff, geomVertCount[g], triIndices.data() + 3 * (size_t)triOff, 3 * (size_t)geomTriCount[g], 0, 16) == 0xFFFFFFFFu) return HPT_ERR_ARG;
    }
    rc = hpt_clear_scene(ctx); if (rc) return rc;
    for (size_t i = 0; i < instGeomId.size(); i++) {
      uint32_t id;
      if (normMatrices2Offs && instHasMotion[i]) {                            // AddInstanceMotion(geomId, {matrix, matrix_motion}, 2) (:864-868)
        float two[32]; std::memcpy(two, instMatrices.data() + 16 * i, 64); std::memcpy(two + 16, instMatricesMotion.data() + 16 * i, 64);
        id = hpt_add_instance_motion(ctx, instGeomId[i], two, 2);
      } else id = hpt_add_instance(ctx, instGeomId[i], instMatrices.data() + 16 * i);
      if (id == 0xFFFFFFFFu) return HPT_ERR_ARG;
    }
    rc = hpt_commit_scene(ctx, 4); if (rc) return rc;
    hpt_scene_desc d = desc();
    rc = hpt_upload_scene(ctx, &d); if (rc) return rc;
    hpt_params p = params(integratorType);
    rc = hpt_update_params(ctx, &p); if (rc) return rc;
    rc = hpt_set_optics(ctx, lensLines.empty() ? nullptr : lensLines.data(), (uint32_t)(lensLines.size() / 4), physSize[0], physSize[1]); if (rc) return rc;
    rc = hpt_pack_xy(ctx, (uint32_t)width, (uint32_t)height); if (rc) return rc;
    return hpt_init_random_gens(ctx, (uint32_t)(width * height));
  }
};

namespace detail {

inline bool readFile(const std::string& path, std::vector<uint8_t>& out)
{
  std::ifstream f(path, std::ios::binary); if (!f) return false;
  f.seekg(0, std::ios::end); const std::streamoff n = f.tellg(); f.seekg(0);
  out.resize((size_t)n); if (n) f.read((char*)out.data(), n);
  return (bool)f;
}

inline Material blankMaterial()
{
  Material m; std::memset(&m, 0, sizeof(m));
  m.lightId = 0xFFFFFFFFu;
  m.texid[0] = 0; m.texid[1] = 0xFFFFFFFFu; m.texid[2] = 0; m.texid[3] = 0;          // texid[1] = no normal map (integrator_pt_scene.cpp:604)
  for (int k = 0; k < 4; k++) { m.spdid[k] = 0xFFFFFFFFu; m.row0[k][0] = 1.0f; m.row1[k][1] = 1.0f; }
  return m;
}
inline LightSource blankLight()
{
  LightSource l; std::memset(&l, 0, sizeof(l));
  l.distType = 0; l.iesId = l.texId = l.specId = l.camBackTexId = l.matId = 0xFFFFFFFFu;
  l.samplerRow0[0] = 1.0f; l.samplerRow1[1] = 1.0f; l.mult = 1.0f;
  return l;
}
inline void lightFrame(const M4& m, LightSource& l)          // pos = M (0,0,0,1), norm = normalize(M (0,-1,0,0))
{
  for (int k = 0; k < 4; k++) l.pos[k] = (float)m.m[k][3];
  const double n[4] = { -m.m[0][1], -m.m[1][1], -m.m[2][1], -m.m[3][1] };
  const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] + n[3] * n[3]);
  for (int k = 0; k < 4; k++) l.norm[k] = (float)(n[k] / len);
}
inline double colLen(const M4& m, int c) { return std::sqrt(m.m[0][c] * m.m[0][c] + m.m[1][c] * m.m[1][c] + m.m[2][c] * m.m[2][c]); }

// CreateSphericalTextureFromIES, axially symmetric photometry, normalised to max 1 (integrator_pt_scene_lgt.cpp:171-186)
// ---- LDR image files of LoadTextureAndMakeCombined (integrator_pt_scene_tex.cpp:24-33: .png / .ppm / .bmp through LiteImage::LoadImage<uint32_t>) ----
// RGBA8 texels, r in the low byte, rows in FILE order (PNG / PPM: top row first; BMP: as stored, bottom row first unless its height is negative).
// LiteImage is absent from the tree, so the row order it hands out is unpinned; .jpg / .jpeg: jpeg_decode.h.
static const uint64_t kMaxImagePixels = uint64_t(1) << 28;                  // every reader refuses larger images before it allocates (the JPEG reader's limit)
inline uint32_t be32(const uint8_t* p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | uint32_t(p[3]); }
inline bool decodePng(const std::vector<uint8_t>& f, uint32_t& w, uint32_t& h, std::vector<uint8_t>& rgba, std::string& err)
{
  static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
  if (f.size() < 33 || std::memcmp(f.data(), sig, 8) != 0) { err = "not a PNG file"; return false; }
  std::vector<uint8_t> idat, plte, trns; uint8_t depth = 0, ctype = 0, interlace = 0; w = h = 0;
  for (size_t p = 8; p + 12 <= f.size();) {
    const uint32_t len = be32(&f[p]); const std::string type((const char*)&f[p + 4], 4);
    if (p + 12 + (size_t)len > f.size()) { err = "PNG truncated"; return false; }
    const uint8_t* d = &f[p + 8];
    if (type == "IHDR" && len >= 13) { w = be32(d); h = be32(d + 4); depth = d[8]; ctype = d[9]; interlace = d[12]; }
    else if (type == "PLTE") plte.assign(d, d + len);
    else if (type == "tRNS") trns.assign(d, d + len);
    else if (type == "IDAT") idat.insert(idat.end(), d, d + len);
    else if (type == "IEND") break;
    p += 12 + (size_t)len;
  }
  if (w == 0 || h == 0 || depth != 8 || interlace != 0 || (ctype != 0 && ctype != 2 && ctype != 3 && ctype != 4 && ctype != 6)) { err = "PNG: only 8-bit non-interlaced images are read"; return false; }
  if ((uint64_t)w * h > kMaxImagePixels) { err = "PNG: unreasonable size"; return false; }   // (a 60-byte file can claim 2^32 x 2^32)
  const uint32_t ch = ctype == 0 ? 1u : ctype == 2 ? 3u : ctype == 3 ? 1u : ctype == 4 ? 2u : 4u;
  const size_t stride = (size_t)w * ch;
  std::vector<uint8_t> raw((stride + 1) * h);
  uLongf outLen = (uLongf)raw.size();
  if (uncompress(raw.data(), &outLen, idat.data(), (uLong)idat.size()) != Z_OK || outLen != raw.size()) { err = "PNG: inflate failed"; return false; }
  std::vector<uint8_t> img(stride * h);
  for (uint32_t y = 0; y < h; y++) {                                          // undo the scanline filters (PNG spec 9)
    const uint8_t ft = raw[(stride + 1) * y]; const uint8_t* in = &raw[(stride + 1) * y + 1];
    uint8_t* out = &img[stride * y]; const uint8_t* up = y ? &img[stride * (y - 1)] : nullptr;
    for (size_t x = 0; x < stride; x++) {
      const int a = x >= ch ? out[x - ch] : 0, b = up ? up[x] : 0, c = (up && x >= ch) ? up[x - ch] : 0;
      int pred = 0;
      if (ft == 1) pred = a; else if (ft == 2) pred = b; else if (ft == 3) pred = (a + b) >> 1;
      else if (ft == 4) { const int pp = a + b - c, pa = std::abs(pp - a), pb = std::abs(pp - b), pc = std::abs(pp - c); pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); }
      else if (ft != 0) { err = "PNG: bad filter type"; return false; }
      out[x] = (uint8_t)(in[x] + pred);
    }
  }
  rgba.resize((size_t)w * h * 4);
  for (size_t i = 0; i < (size_t)w * h; i++) {
    const uint8_t* s = &img[i * ch]; uint8_t* o = &rgba[4 * i];
    if (ctype == 0) { o[0] = o[1] = o[2] = s[0]; o[3] = 255; }
    else if (ctype == 2) { o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = 255; }
    else if (ctype == 3) { const size_t k = s[0]; if (3 * k + 2 >= plte.size()) { err = "PNG: palette index out of range"; return false; } o[0] = plte[3 * k]; o[1] = plte[3 * k + 1]; o[2] = plte[3 * k + 2]; o[3] = k < trns.size() ? trns[k] : 255; }
    else if (ctype == 4) { o[0] = o[1] = o[2] = s[0]; o[3] = s[1]; }
    else { o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = s[3]; }
  }
  return true;
}
inline bool decodePpm(const std::vector<uint8_t>& f, uint32_t& w, uint32_t& h, std::vector<uint8_t>& rgba, std::string& err)
{
  size_t p = 0; auto token = [&]() { std::string t; while (p < f.size()) { if (f[p] == '#') { while (p < f.size() && f[p] != '\n') p++; } else if (std::isspace(f[p])) { if (!t.empty()) break; p++; } else t.push_back((char)f[p++]); } return t; };
  if (token() != "P6") { err = "PPM: only binary P6 is read"; return false; }
  w = (uint32_t)std::atoll(token().c_str()); h = (uint32_t)std::atoll(token().c_str()); const int maxv = std::atoi(token().c_str());
  p++;                                                                        // the single whitespace byte after the header
  if (w == 0 || h == 0 || maxv != 255 || (uint64_t)w * h > kMaxImagePixels || p + (size_t)w * h * 3 > f.size()) { err = "PPM: bad header or truncated"; return false; }
  rgba.resize((size_t)w * h * 4);
  for (size_t i = 0; i < (size_t)w * h; i++) { rgba[4 * i] = f[p + 3 * i]; rgba[4 * i + 1] = f[p + 3 * i + 1]; rgba[4 * i + 2] = f[p + 3 * i + 2]; rgba[4 * i + 3] = 255; }
  return true;
}
inline bool decodeBmp(const std::vector<uint8_t>& f, uint32_t& w, uint32_t& h, std::vector<uint8_t>& rgba, std::string& err)
{
  if (f.size() < 54 || f[0] != 'B' || f[1] != 'M') { err = "not a BMP file"; return false; }
  uint32_t off; int32_t sw, sh; uint16_t bpp; uint32_t comp;
  std::memcpy(&off, &f[10], 4); std::memcpy(&sw, &f[18], 4); std::memcpy(&sh, &f[22], 4); std::memcpy(&bpp, &f[28], 2); std::memcpy(&comp, &f[30], 4);
  if (sw <= 0 || sh == 0 || sh == INT32_MIN || (bpp != 24 && bpp != 32) || (comp != 0 && comp != 3)) { err = "BMP: only uncompressed 24 / 32-bit images are read"; return false; }
  w = (uint32_t)sw; h = (uint32_t)(sh < 0 ? -sh : sh);
  if ((uint64_t)w * h > kMaxImagePixels) { err = "BMP: unreasonable size"; return false; }
  const size_t stride = (((size_t)w * (bpp / 8)) + 3) & ~size_t(3);
  if (off + stride * h > f.size()) { err = "BMP truncated"; return false; }
  rgba.resize((size_t)w * h * 4);
  for (uint32_t y = 0; y < h; y++) for (uint32_t x = 0; x < w; x++) {         // rows as stored (bottom-up for a positive height)
    const uint8_t* s = &f[off + stride * y + (size_t)x * (bpp / 8)]; uint8_t* o = &rgba[4 * ((size_t)y * w + x)];
    o[0] = s[2]; o[1] = s[1]; o[2] = s[0]; o[3] = bpp == 32 ? s[3] : 255;
  }
  return true;
}
// OpenEXR, the subset the reference reads through tinyexr's LoadEXR (imageutils.cpp:317-392): single-part scanline files, NONE / ZIPS / ZIP
// compression, HALF / FLOAT / UINT channels. rgba: w * h * 4 floats in FILE order (top scanline first), as LoadEXR hands them out:
// R, G, B (, A = 1 when absent); a single-channel file fills all four components with its value.
inline float halfToFloat(uint16_t hbits)
{
  const uint32_t sign = (uint32_t)(hbits & 0x8000u) << 16, exp = (hbits >> 10) & 0x1Fu, man = hbits & 0x3FFu;
  uint32_t f;
  if (exp == 0) {
    if (man == 0) f = sign;
    else { int e = -1; uint32_t m = man; do { e++; m <<= 1; } while (!(m & 0x400u)); f = sign | ((uint32_t)(127 - 15 - e) << 23) | ((m & 0x3FFu) << 13); }   // subnormal
  } else if (exp == 31) f = sign | 0x7F800000u | (man << 13);
  else f = sign | ((exp + 112u) << 23) | (man << 13);
  float r; std::memcpy(&r, &f, 4); return r;
}
inline bool decodeExr(const std::vector<uint8_t>& f, uint32_t& w, uint32_t& h, std::vector<float>& rgba, std::string& err)
{
  static const uint8_t magic[4] = { 0x76, 0x2f, 0x31, 0x01 };
  if (f.size() < 16 || std::memcmp(f.data(), magic, 4) != 0) { err = "exr: not an OpenEXR file"; return false; }
  uint32_t version; std::memcpy(&version, f.data() + 4, 4);
  if (version & 0x1A00u) { err = "exr: tiled / multi-part / deep files are not read"; return false; }
  size_t p = 8;
  struct Chan { std::string name; int type; };
  std::vector<Chan> chans; int comp = -1; int32_t dw[4] = {0, 0, -1, -1};
  auto cstr = [&](size_t& q, const std::vector<uint8_t>& b, size_t end, std::string& out) { out.clear(); while (q < end && b[q] != 0) out.push_back((char)b[q++]); q++; return q <= end; };
  while (p < f.size() && f[p] != 0) {
    std::string name, type;
    if (!cstr(p, f, f.size(), name) || !cstr(p, f, f.size(), type) || p + 4 > f.size()) { err = "exr: broken header"; return false; }
    int32_t size; std::memcpy(&size, f.data() + p, 4); p += 4;
    if (size < 0 || p + (size_t)size > f.size()) { err = "exr: broken header"; return false; }
    if (name == "channels") {
      size_t q = p; const size_t end = p + (size_t)size;
      while (q < end && f[q] != 0) {
        Chan c; if (!cstr(q, f, end, c.name) || q + 16 > end) { err = "exr: broken channel list"; return false; }
        int32_t pt, xs, ys; std::memcpy(&pt, f.data() + q, 4); std::memcpy(&xs, f.data() + q + 8, 4); std::memcpy(&ys, f.data() + q + 12, 4); q += 16;
        if (xs != 1 || ys != 1 || pt < 0 || pt > 2) { err = "exr: subsampled channels are not read"; return false; }
        c.type = pt; chans.push_back(c);
      }
    } else if (name == "compression" && size >= 1) comp = f[p];
    else if (name == "dataWindow" && size == 16) std::memcpy(dw, f.data() + p, 16);
    p += (size_t)size;
  }
  p++;
  const int lpb = comp == 0 ? 1 : (comp == 2 ? 1 : (comp == 3 ? 16 : 0));
  if (!lpb) { err = "exr: compression " + std::to_string(comp) + " is not read (NONE, ZIPS, ZIP are)"; return false; }
  if (chans.empty() || dw[2] < dw[0] || dw[3] < dw[1]) { err = "exr: no channels / empty data window"; return false; }
  w = (uint32_t)(dw[2] - dw[0] + 1); h = (uint32_t)(dw[3] - dw[1] + 1);
  if (w > 65536u || h > 65536u || (uint64_t)w * h > kMaxImagePixels) { err = "exr: unreasonable size"; return false; }
  const size_t nblocks = (h + (uint32_t)lpb - 1) / (uint32_t)lpb;
  if (p + 8 * nblocks > f.size()) { err = "exr: truncated offset table"; return false; }
  size_t lineBytes = 0; for (const Chan& c : chans) lineBytes += (c.type == 1 ? 2u : 4u) * (size_t)w;
  // before the planes are allocated: an uncompressed file holds every line, a compressed one at least a chunk header per block
  if ((comp == 0 && (uint64_t)lineBytes * h > f.size()) || 8 * (uint64_t)nblocks > f.size()) { err = "exr: file shorter than its header says"; return false; }
  std::vector<std::vector<float>> planes(chans.size(), std::vector<float>((size_t)w * h, 0.0f));
  std::vector<uint8_t> tmp, raw;
  for (size_t b = 0; b < nblocks; b++) {
    uint64_t off; std::memcpy(&off, f.data() + p + 8 * b, 8);
    if (f.size() < 8 || off > f.size() - 8) { err = "exr: chunk offset past the end"; return false; }      // (not off + 8 > size: an offset near 2^64 wraps)
    int32_t y, size; std::memcpy(&y, f.data() + off, 4); std::memcpy(&size, f.data() + off + 4, 4);
    if (size < 0 || (uint64_t)size > f.size() - 8 - off || y < dw[1] || y > dw[3]) { err = "exr: broken chunk"; return false; }
    const size_t nl = (size_t)std::min<int64_t>(lpb, (int64_t)dw[3] - y + 1), need = nl * lineBytes;
    const uint8_t* data = f.data() + off + 8;
    if (comp != 0 && (size_t)size < need) {
      tmp.resize(need); uLongf got = (uLongf)need;
      if (uncompress(tmp.data(), &got, data, (uLong)size) != Z_OK || got != need) { err = "exr: zlib"; return false; }
      for (size_t i = 1; i < need; i++) tmp[i] = (uint8_t)(tmp[i - 1] + tmp[i] - 128);        // predictor
      raw.resize(need);
      const size_t half = (need + 1) / 2;
      for (size_t i = 0, a = 0, c = half; i < need;) { raw[i++] = tmp[a++]; if (i < need) raw[i++] = tmp[c++]; }   // the two byte halves interleaved again
      data = raw.data();
    } else if ((size_t)size < need) { err = "exr: short chunk"; return false; }
    size_t q = 0;
    for (size_t l = 0; l < nl; l++) for (size_t ci = 0; ci < chans.size(); ci++) {
      float* dst = planes[ci].data() + ((size_t)(y - dw[1]) + l) * w;
      for (uint32_t x = 0; x < w; x++) {
        if (chans[ci].type == 1) { uint16_t v; std::memcpy(&v, data + q, 2); q += 2; dst[x] = halfToFloat(v); }
        else if (chans[ci].type == 2) { std::memcpy(&dst[x], data + q, 4); q += 4; }
        else { uint32_t v; std::memcpy(&v, data + q, 4); q += 4; dst[x] = (float)v; }
      }
    }
  }
  rgba.assign((size_t)w * h * 4, 0.0f);
  auto find = [&](const char* n) -> const float* { for (size_t ci = 0; ci < chans.size(); ci++) if (chans[ci].name == n) return planes[ci].data(); return nullptr; };
  if (chans.size() == 1) { for (size_t i = 0; i < (size_t)w * h; i++) for (int k = 0; k < 4; k++) rgba[4 * i + k] = planes[0][i]; return true; }
  const float* src[4] = { find("R"), find("G"), find("B"), find("A") };
  for (size_t i = 0; i < (size_t)w * h; i++) for (int k = 0; k < 4; k++) rgba[4 * i + k] = src[k] ? src[k][i] : (k == 3 ? 1.0f : 0.0f);
  return true;
}

inline bool endsWithNoCase(const std::string& s, const char* ext) { const size_t n = std::strlen(ext); if (s.size() < n) return false; for (size_t i = 0; i < n; i++) if (std::tolower((unsigned char)s[s.size() - n + i]) != ext[i]) return false; return true; }

// ---- spectra (spectrum.cpp) ----
static const float kLambdaMin = 360.0f, kLambdaMax = 830.0f;            // include/cglobals.h:22-23
// Spectrum::ResampleUniform over Spectrum::Sample (spectrum.cpp:7-48): 471 values at LAMBDA_MIN + c nm, zero outside the tabulated range,
// linear in between - in float, as the reference evaluates it
inline std::vector<float> resampleUniform(const std::vector<float>& w, const std::vector<float>& v)
{
  std::vector<float> out((size_t)(kLambdaMax - kLambdaMin + 1.0f), 0.0f);
  if (w.size() < 2 || v.size() < w.size()) return out;                   // (an .spd with fewer than two samples: the reference indexes w[-1] there; here the spectrum reads zero)
  for (size_t c = 0; c < out.size(); c++) {
    const float lam = kLambdaMin + float(c);
    if (lam < w.front() || lam > w.back()) continue;
    int last = (int)w.size() - 2, first = 1;                            // BinarySearch (spectrum.h:26-40)
    while (last > 0) {
      const int half = last >> 1, middle = first + half;
      if (w[(size_t)middle] <= lam) { first = middle + 1; last = last - (half + 1); } else last = half;
    }
    const int o = std::min(std::max(first - 1, 0), (int)w.size() - 2);
    const float t = (lam - w[(size_t)o]) / (w[(size_t)o + 1] - w[(size_t)o]);
    out[c] = v[(size_t)o] + t * (v[(size_t)o + 1] - v[(size_t)o]);
  }
  return out;
}
// LoadSPDFromFile (spectrum.cpp:50-71): "lambda value" per line, '#' comments
inline bool loadSpd(const std::string& path, std::vector<float>& w, std::vector<float>& v)
{
  std::vector<uint8_t> raw; if (!readFile(path, raw)) return false;
  std::istringstream is(std::string(raw.begin(), raw.end())); std::string line;
  while (std::getline(is, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    const size_t sp = line.find(' ');
    if (sp == std::string::npos) continue;
    w.push_back((float)std::atof(line.substr(0, sp).c_str())); v.push_back((float)std::atof(line.substr(sp + 1).c_str()));
  }
  return true;
}
inline bool iesSphericalTexture(const std::string& path, LoadedTexture& tex, std::string& err)
{
  std::vector<uint8_t> raw; if (!readFile(path, raw)) { err = "cannot read " + path; return false; }
  const std::string s(raw.begin(), raw.end());
  const size_t p = s.find("TILT=NONE"); if (p == std::string::npos) { err = "IES: only TILT=NONE files are handled"; return false; }
  const std::vector<double> vals = parseFloats(s.substr(p + 9));
  if (vals.size() < 13) { err = "IES: truncated header"; return false; }
  const int nVert = (int)vals[3], nHorz = (int)vals[4];
  if (nHorz != 1) { err = "IES: only axially symmetric photometry (one horizontal angle) is handled"; return false; }
  if ((int)vals.size() < 13 + nVert + nHorz + nVert) { err = "IES: truncated data"; return false; }
  const double* vert = vals.data() + 13; const double* cand = vert + nVert + nHorz;
  const double v0 = vert[0], v1 = vert[nVert - 1];
  const bool half = (std::fabs(v0) < 1e-5 && std::fabs(v1 - 90) < 1e-5) || (std::fabs(v0 - 90) < 1e-5 && std::fabs(v1 - 180) < 1e-5);
  const int h = half ? nVert * 2 : nVert;
  std::vector<float> img((size_t)h, 0.0f);
  const float step = float(v1 - v0) / float(nVert);
  float thetaGrad = float(v0);
  for (int ti = 0; ti < nVert; ti++) {
    const float theta = float(M_PI / 180.0) * thetaGrad;
    int iy = int((theta * float(1.0 / M_PI)) * float(h) + 0.5f); if (iy > h - 1) iy = h - 1;
    img[(size_t)iy] = (float)cand[ti];
    thetaGrad = thetaGrad + step;
  }
  float mx = 0.0f; for (float v : img) mx = std::max(mx, v); if (mx == 0.0f) mx = 1.0f;
  const float inv = 1.0f / mx; for (float& v : img) v *= inv;
  tex = LoadedTexture(); tex.width = 1; tex.height = (uint32_t)h; tex.format = 2; tex.flags = 0; tex.addressU = 2; tex.addressV = 2; tex.filter = 1;
  tex.bytes.resize(img.size() * 4); std::memcpy(tex.bytes.data(), img.data(), tex.bytes.size());
  return true;
}

} // namespace detail

// Mesh4fInput (integrator_pt.h:103-119): a mesh handed over as pointers instead of a .vsgf file - what Integrator::LoadScene_SetMeshPointers
// (:154) receives from the HR2 render driver (hydra_api/hydra_cpu.cpp:36-70) and LoadSceneGeometry reads for <mesh ... ptrs="1"> nodes
// (integrator_pt_scene.cpp:750-789). Same member names and meaning.
struct Mesh4fInput
{
  const float*    vPosPtr = nullptr; uint32_t vPosByteStride = 16;
  const float*    vNormPtr4f = nullptr; const float* vTangPtr4f = nullptr; const float* vTexCoord2f = nullptr;
  const uint32_t* indicesPtr = nullptr; uint32_t indicesNum = 0, vertNum = 0;
  const uint32_t* matIdPtr = nullptr; uint32_t matIdAll = 0, matIdNum = 1;       // matIdNum != indicesNum / 3: the whole mesh takes matIdAll
};

inline bool LoadHydraXmlText(const std::string& text, const std::string& folder, int width, int height, LoadedScene& sc, std::string& err, bool spectral = false,
                             const std::unordered_map<int, Mesh4fInput>* meshPtrs = nullptr);

inline bool LoadHydraXml(const std::string& xmlPath, int width, int height, LoadedScene& sc, std::string& err, bool spectral = false,
                         const std::unordered_map<int, Mesh4fInput>* meshPtrs = nullptr)
{
  std::vector<uint8_t> raw; if (!detail::readFile(xmlPath, raw)) { err = "cannot read " + xmlPath; return false; }
  const size_t slash = xmlPath.find_last_of("/\\");
  return LoadHydraXmlText(std::string(raw.begin(), raw.end()), slash == std::string::npos ? std::string(".") : xmlPath.substr(0, slash), width, height, sc, err, spectral, meshPtrs);
}

// the scene description as TEXT (an HR2 client keeps it in memory: hydra_api's xmlData) + the folder its relative paths start from
inline bool LoadHydraXmlText(const std::string& text, const std::string& folder, int width, int height, LoadedScene& sc, std::string& err, bool spectral,
                             const std::unordered_map<int, Mesh4fInput>* meshPtrs)
{
  using namespace detail;
  XmlNode root; XmlParser parser(text); if (!parser.parse(root, err)) return false;
  sc = LoadedScene();
  {                                                         // m_textures[0]: 1x1 white, NEAREST / CLAMP (integrator_pt_scene_tex.cpp:7-16)
    LoadedTexture w; w.width = w.height = 1; w.format = 0; w.flags = 0; w.addressU = w.addressV = 2; w.filter = 0; w.bytes.assign(4, 0xFF);
    sc.textures.push_back(w);
  }
  const XmlNode* settings = root.path("render_lib/render_settings");
  const XmlNode* cam = root.path("cam_lib/camera");
  const XmlNode* sceneNode = root.path("scenes/scene");
  if (!settings || !cam || !sceneNode) { err = "xml: render_settings / camera / scene missing"; return false; }
  auto toInt = [](const std::string& s) { return s.empty() ? 0 : std::atoi(s.c_str()); };
  sc.width = width > 0 ? width : toInt(settings->childText("width"));
  sc.height = height > 0 ? height : toInt(settings->childText("height"));
  sc.traceDepth = toInt(settings->childText("trace_depth")) ? (uint32_t)toInt(settings->childText("trace_depth")) : 6u;          // LoadSceneSettings :926-940
  sc.spp = toInt(settings->childText("maxRaysPerPixel")) ? (uint32_t)toInt(settings->childText("maxRaysPerPixel")) : 1u;
  sc.fov = std::atof(cam->childText("fov").c_str());
  sc.nearClip = std::atof(cam->childText("nearClipPlane").c_str()); sc.farClip = std::atof(cam->childText("farClipPlane").c_str());
  { const auto p = parseFloats(cam->childText("position")), l = parseFloats(cam->childText("look_at")), u = parseFloats(cam->childText("up"));
    if (p.size() < 3 || l.size() < 3 || u.size() < 3) { err = "xml: camera vectors"; return false; }
    for (int k = 0; k < 3; k++) { sc.camPos[k] = p[k]; sc.camLookAt[k] = l[k]; sc.camUp[k] = u[k]; } }

  // lens simulation: LoadOpticsFromNode (integrator_pt_scene.cpp:1078-1141). The reference reads m_aspect there before anything has set it;
  // height / width of the frame is taken (the film's aspect in pbrt's RealisticCamera, which the code follows). Its fallback to an <optics>
  // node never triggers (opticNode != opticNode).
  if (const XmlNode* optics = cam->child("optical_system")) {
    const float scale = optics->has("scale") ? (float)std::atof(optics->get("scale").c_str()) : 1.0f;
    const float diagonal = optics->has("sensor_diagonal") ? (float)std::atof(optics->get("sensor_diagonal").c_str()) : 0.035f;
    struct Line { int id; float r, t, ior, ap; };
    std::vector<Line> lines; int k = 0;
    for (const XmlNode* ln : optics->all("line")) {
      Line l; l.id = ln->has("id") ? std::atoi(ln->get("id").c_str()) : k;
      l.r = scale * (float)std::atof(ln->get("curvature_radius", "0").c_str()); l.t = scale * (float)std::atof(ln->get("thickness", "0").c_str());
      l.ior = (float)std::atof(ln->get("ior", "0").c_str());
      l.ap = scale * (float)std::atof((ln->has("semi_diameter") ? ln->get("semi_diameter") : ln->get("aperture_radius", "0")).c_str());
      lines.push_back(l); k++;
    }
    const bool desc = optics->get("order") == "scene_to_sensor";
    std::stable_sort(lines.begin(), lines.end(), [desc](const Line& a, const Line& b) { return desc ? a.id > b.id : a.id < b.id; });
    for (const Line& l : lines) { sc.lensLines.push_back(l.r); sc.lensLines.push_back(l.t); sc.lensLines.push_back(l.ior); sc.lensLines.push_back(l.ap); }
    const float aspect = float(sc.height) / float(sc.width);
    sc.physSize[0] = 2.0f * std::sqrt(diagonal * diagonal / (1.0f + aspect * aspect)); sc.physSize[1] = aspect * sc.physSize[0];
  }

  // textures: LoadSceneTexturesInfo (integrator_pt_scene.cpp:330-355) keeps the nodes with a size, indexed by position; a <texture id=..> is
  // loaded on first use, one table entry per distinct (id, address modes, filter) - the HydraSampler equality of integrator_pt.h:75-83
  // (rows and gamma are not part of the key) - LoadTextureFromNode, integrator_pt_scene_tex.cpp:105-126
  struct TexInfo { std::string path; uint32_t w, h, bpp; };
  std::vector<TexInfo> texInfo;
  if (const XmlNode* lib = root.child("textures_lib")) for (const XmlNode* t : lib->all("texture")) {
    const uint32_t w = (uint32_t)std::atoll(t->get("width", "0").c_str()), h = (uint32_t)std::atoll(t->get("height", "0").c_str());
    if (w == 0 || h == 0) continue;
    TexInfo ti; ti.path = t->get("loc").empty() ? t->get("path") : folder + "/" + t->get("loc"); ti.w = w; ti.h = h;
    ti.bpp = (uint32_t)((uint64_t)std::atoll(t->get("bytesize", "0").c_str()) / ((uint64_t)w * h));
    texInfo.push_back(ti);
  }
  std::map<std::array<uint32_t, 5>, uint32_t> texCache;
  // ReadSamplerFromColorNode (integrator_pt_scene_mat.cpp:32-91) + LoadTextureFromNode: rows of the node's sampler and the table index
  // (childName / forceXid / forceNoGamma: LoadSpectralTextures reads the sampler from the colour node's <spectrum> child, names the texture itself
  // and never applies gamma - integrator_pt_scene_mat.cpp:144-173, LoadTextureById integrator_pt_scene_tex.cpp:129-144)
  auto loadTex = [&](const XmlNode* node, const char* childName, int forceXid, bool forceNoGamma, float* row0, float* row1, uint32_t& outId) -> bool {
    outId = 0;
    row0[0] = 1.0f; row0[1] = row0[2] = row0[3] = 0.0f; row1[0] = 0.0f; row1[1] = 1.0f; row1[2] = row1[3] = 0.0f;
    const XmlNode* tn = node ? node->child(childName) : nullptr;
    if (!tn) return true;
    bool bad = false;
    auto addr = [&](const char* name, uint32_t dflt) -> uint32_t {
      if (!tn->has(name)) return dflt;
      const std::string v = tn->get(name);
      if (v == "clamp") return 2u;
      if (v == "mirror" || v == "border" || v == "mirror_once") { bad = true; return 0u; }
      return 0u;                                                              // "wrap" and anything else
    };
    const uint32_t au = addr("addressing_mode_u", 0u), av = addr("addressing_mode_v", 0u), aw = addr("addressing_mode_w", av);
    if (bad) { err = "xml: texture addressing modes other than wrap / clamp are outside the path"; return false; }
    uint32_t filt = 1u;
    const std::string fm = tn->get("filter");
    if (fm == "point" || fm == "nearest") filt = 0u;
    else if (fm == "cubic" || fm == "bicubic") { err = "xml: bicubic texture filtering is outside the path"; return false; }
    { const auto mv = parseFloats(tn->get("matrix")); for (size_t i = 0; i < mv.size() && i < 8; i++) (i < 4 ? row0 : row1)[i % 4] = (float)mv[i]; }
    const bool disableGamma = forceNoGamma || (tn->has("input_gamma") && (int)std::atof(tn->get("input_gamma").c_str()) == 1);
    const uint32_t xid = forceXid >= 0 ? (uint32_t)forceXid : (uint32_t)std::atoi(tn->get("id").c_str());
    const std::array<uint32_t, 5> key = { xid, au, av, aw, filt };
    auto it = texCache.find(key); if (it != texCache.end()) { outId = it->second; return true; }
    if (xid >= texInfo.size()) { err = "xml: texture id not in textures_lib"; return false; }
    const TexInfo& ti = texInfo[xid];
    std::vector<uint8_t> img;
    if (!readFile(ti.path, img) || img.size() < 8) { err = "cannot read " + ti.path; return false; }
    LoadedTexture t; t.addressU = au; t.addressV = av; t.filter = filt;
    if (ti.path.find(".exr") != std::string::npos) {                          // LoadImage4fFromEXR / LoadImage1fFromEXR (imageutils.cpp:317-392): tinyexr's rows, flipped
      uint32_t w = 0, h = 0; std::vector<float> rgba; std::string derr;
      if (!decodeExr(img, w, h, rgba, derr)) { err = "texture file '" + ti.path + "': " + derr; return false; }
      t.width = w; t.height = h; t.flags = 0u;
      if (ti.bpp == 16) {
        t.format = 1u; t.bytes.resize((size_t)w * h * 16);
        for (uint32_t y = 0; y < h; y++) std::memcpy(t.bytes.data() + (size_t)(h - 1 - y) * w * 16, rgba.data() + (size_t)y * w * 4, (size_t)w * 16);
      } else {                                                               // one float per texel: R, infinities and values beyond the half range clamped
        t.format = 2u; t.bytes.resize((size_t)w * h * 4);
        for (uint32_t y = 0; y < h; y++) for (uint32_t x = 0; x < w; x++) {
          float v = rgba[((size_t)(h - 1 - y) * w + x) * 4];
          v = std::isinf(v) ? 65504.0f : std::min(std::max(v, 0.0f), 65504.0f);
          std::memcpy(t.bytes.data() + ((size_t)y * w + x) * 4, &v, 4);
        }
      }
    } else if (ti.path.find(".image") == std::string::npos) {                 // LDR files through LiteImage::LoadImage<uint32_t> (:24-33)
      uint32_t w = 0, h = 0; std::vector<uint8_t> rgba; std::string derr;
      const bool ok = endsWithNoCase(ti.path, ".png") ? decodePng(img, w, h, rgba, derr) : endsWithNoCase(ti.path, ".ppm") ? decodePpm(img, w, h, rgba, derr)
                    : endsWithNoCase(ti.path, ".bmp") ? decodeBmp(img, w, h, rgba, derr) : (endsWithNoCase(ti.path, ".jpg") || endsWithNoCase(ti.path, ".jpeg")) ? jpeg::decode(img, w, h, rgba, derr)
                    : (derr = "only .image4ub / .image4f / .exr / .png / .jpg / .ppm / .bmp are read here", false);
      if (!ok) { err = "texture file '" + ti.path + "': " + derr; return false; }
      t.width = w; t.height = h; t.format = 0u; t.flags = disableGamma ? 0u : 1u; t.bytes.swap(rgba);
    } else {
    uint32_t w, h; std::memcpy(&w, img.data(), 4); std::memcpy(&h, img.data() + 4, 4);          // {w, h} then the texels (integrator_pt_scene_tex.cpp:53-93)
    if (w == 0 || h == 0) {                                                  // white float dummy (:67-73)
      t.width = t.height = 1; t.format = 1; t.flags = 0; const float one[4] = {1, 1, 1, 1}; t.bytes.assign((const uint8_t*)one, (const uint8_t*)one + 16);
    } else {
      const size_t texel = ti.bpp == 16 ? 16 : 4;
      if (img.size() < 8 + (size_t)w * h * texel) { err = "image truncated: " + ti.path; return false; }
      t.width = w; t.height = h; t.format = ti.bpp == 16 ? 1u : 0u; t.flags = (ti.bpp != 16 && !disableGamma) ? 1u : 0u;
      t.bytes.assign(img.begin() + 8, img.begin() + 8 + (size_t)w * h * texel);
    }
    }
    sc.textures.push_back(std::move(t));
    outId = texCache[key] = (uint32_t)sc.textures.size() - 1;
    return true;
  };
  auto loadTextureFromNode = [&](const XmlNode* node, float* row0, float* row1, uint32_t& outId) -> bool { return loadTex(node, "texture", -1, false, row0, row1, outId); };
  std::set<uint32_t> loadedSpectral;
  auto loadSpectralTextures = [&](uint32_t specId, const XmlNode* colorNode) -> bool {      // LoadSpectralTextures (integrator_pt_scene_mat.cpp:144-173)
    if (specId == 0xFFFFFFFFu || 2 * (size_t)specId + 1 >= sc.specTexOffsetSz.size() || sc.specTexOffsetSz[2 * specId + 1] == 0u || loadedSpectral.count(specId)) return true;
    const uint32_t off = sc.specTexOffsetSz[2 * specId], n = sc.specTexOffsetSz[2 * specId + 1];
    for (uint32_t k2 = 0; k2 < n; k2++) {
      float r0[4], r1[4]; uint32_t id = 0;
      if (!loadTex(colorNode, "spectrum", (int)sc.specTexIdsWavelengths[2 * (off + k2)], true, r0, r1, id)) return false;
      sc.specTexIdsWavelengths[2 * (off + k2)] = id;
    }
    loadedSpectral.insert(specId);
    return true;
  };

  // LoadSceneSpectrumData (integrator_pt_scene.cpp:358-419): every <spectrum> resampled at 1 nm, one {offset, size} per node in node order
  sc.spectralMode = spectral ? 1u : 0u;
  if (const XmlNode* lib = root.child("spectra_lib")) for (const XmlNode* sn : lib->all("spectrum")) {
    if (sn->has("lambda_ref_ids")) {                                          // given by textures (:363-377): "lambda texture lambda texture ..."
      const auto refs = parseFloats(sn->get("lambda_ref_ids"));
      sc.specTexOffsetSz.push_back((uint32_t)(sc.specTexIdsWavelengths.size() / 2)); sc.specTexOffsetSz.push_back((uint32_t)(refs.size() / 2));
      for (size_t k2 = 0; k2 + 1 < refs.size(); k2 += 2) { sc.specTexIdsWavelengths.push_back((uint32_t)refs[k2 + 1]); sc.specTexIdsWavelengths.push_back((uint32_t)refs[k2]); }
      sc.specOffsetSz.push_back(0xFFFFFFFFu); sc.specOffsetSz.push_back(0u);
      continue;
    }
    sc.specTexOffsetSz.push_back(0xFFFFFFFFu); sc.specTexOffsetSz.push_back(0u);
    std::vector<float> w, v;
    if (sn->has("value")) { const auto nums = parseFloats(sn->get("value")); for (size_t k = 0; k + 1 < nums.size(); k += 2) { w.push_back((float)nums[k]); v.push_back((float)nums[k + 1]); } }
    else if (!loadSpd(folder + "/" + sn->get("loc"), w, v)) { err = "cannot read spectrum " + sn->get("loc"); return false; }
    const std::vector<float> u = resampleUniform(w, v);
    sc.specOffsetSz.push_back((uint32_t)sc.specValues.size()); sc.specOffsetSz.push_back((uint32_t)u.size());
    sc.specValues.insert(sc.specValues.end(), u.begin(), u.end());
  }
  if (sc.specOffsetSz.empty()) {                                              // "if no spectra are loaded add uniform 1.0 spectrum" (:406-418)
    const std::vector<float> u = resampleUniform({200.0f, 400.0f, 600.0f, 800.0f}, {1.0f, 1.0f, 1.0f, 1.0f});
    sc.specOffsetSz.push_back(0u); sc.specOffsetSz.push_back((uint32_t)u.size()); sc.specValues = u;
    sc.specTexOffsetSz.push_back(0xFFFFFFFFu); sc.specTexOffsetSz.push_back(0u);
  }
  sc.cieXYZ = cieXyzFit();
  auto spectrumId = [](const XmlNode* n) -> uint32_t {                        // GetSpectrumIdFromNode (integrator_pt_scene_mat.cpp:109-119)
    const XmlNode* sn = n ? n->child("spectrum") : nullptr;
    return sn ? (uint32_t)std::atoi(sn->get("id").c_str()) : 0xFFFFFFFFu;
  };
  if (const XmlNode* sensor = cam->child("sensor")) if (const XmlNode* resp = sensor->child("response")) {   // integrator_pt_scene.cpp:688-711
    const std::string rt = resp->get("type");
    sc.camResponseType = (rt == "xyz" || rt == "XYZ") ? 0u : 1u;              // CAM_RESPONCE_XYZ = 0, CAM_RESPONCE_RGB = 1
    int id = 0;
    for (const XmlNode* spn : resp->all("spectrum")) { sc.camResponseSpectrumId[id++] = std::atoi(spn->get("id").c_str()); if (id >= 3) break; }
    float rgb[4] = {0, 0, 0, 0};
    if (const XmlNode* cn = resp->child("color")) if (cn->has("val")) {
      const auto cv = parseFloats(cn->get("val"));
      if (cv.size() == 1) rgb[0] = rgb[1] = rgb[2] = (float)cv[0]; else if (cv.size() >= 3) for (int k = 0; k < 3; k++) rgb[k] = (float)cv[k];
    }
    for (int k = 0; k < 3; k++) sc.camRespoceRGB[k] = rgb[k];
    sc.camRespoceRGB[3] = 1.0f;
  }

  // lights first: emissive materials copy intensity from them (integrator_pt_scene.cpp:973-996, 575-599)
  std::map<int, const XmlNode*> lightNodes;
  if (const XmlNode* lib = root.child("lights_lib")) for (const XmlNode* l : lib->all("light")) lightNodes[std::atoi(l->get("id").c_str())] = l;
  std::vector<int> oldToNew;
  for (const XmlNode* linst : sceneNode->all("instance_light")) {
    const int lid = std::atoi(linst->get("light_id").c_str());
    if (!lightNodes.count(lid)) { err = "xml: instance_light refers to an unknown light"; return false; }
    const XmlNode* ln = lightNodes[lid];
    const M4 m = m4FromText(linst->get("matrix"));
    const std::string ltype = ln->get("type"), shape = ln->get("shape"), dist = ln->get("distribution");
    const XmlNode* inten = ln->child("intensity");
    if (!inten || !inten->child("color")) { err = "xml: light without intensity"; return false; }
    auto color = parseFloats(inten->child("color")->get("val"));
    const double power = inten->child("multiplier") ? std::atof(inten->child("multiplier")->get("val").c_str()) : 1.0;
    const bool splat = color.size() == 1;                                     // GetColorFromNode: one value fills all four components
    if (splat) color.assign(4, color[0]);
    if (color.size() < 3) { err = "xml: light colour"; return false; }
    if (ltype == "sky") {                                                     // LIGHT_GEOM_ENV (integrator_pt_scene_lgt.cpp:36-59, integrator_pt_scene.cpp:441-486)
      for (int k = 0; k < 3; k++) sc.envColor[k] = (float)color[k];
      sc.envColor[3] = color.size() >= 4 ? (float)color[3] : 0.0f;
      const XmlNode* cn = inten->child("color");
      sc.envSpecId = spectrumId(cn); sc.envSpecMult = (float)power;          // m_envSpecId = lightSource.specId, m_envSpecMult = lightSource.mult
      float row0[4] = {1, 0, 0, 0}, row1[4] = {0, 1, 0, 0};
      uint32_t envTex = 0xFFFFFFFFu, backTex = 0xFFFFFFFFu;
      bool sample = false;
      if (cn->child("texture")) {
        if (!loadTextureFromNode(cn, row0, row1, envTex)) return false;
        // "m_textureLoadInfo[lightSource.texId]": the reference indexes the XML table with the loaded-texture index (:460-461)
        sample = envTex < texInfo.size() && (texInfo[envTex].path.find(".exr") != std::string::npos || texInfo[envTex].bpp > 4);
      }
      if (const XmlNode* back = ln->child("back")) { float r0[4], r1[4]; if (!loadTextureFromNode(back, r0, r1, backTex)) return false; }
      for (int k = 0; k < 4; k++) { sc.envSamRow0[k] = row0[k]; sc.envSamRow1[k] = row1[k]; }
      sc.envTexId = envTex; sc.envCamBackId = backTex; sc.envLightId = 0xFFFFFFFFu; sc.envEnableSam = (envTex != 0xFFFFFFFFu && sample) ? 1u : 0u;
      if (!sc.envEnableSam) { oldToNew.push_back(-1); continue; }            // a plain-colour or LDR environment is not a light to sample
      const LoadedTexture& tex = sc.textures[envTex];
      if (tex.format != 1) { err = "xml: a sampled environment map must be a float4 image"; return false; }
      LightSource lt = blankLight();
      for (int k = 0; k < 4; k++) { lt.intensity[k] = sc.envColor[k]; lt.samplerRow0[k] = row0[k]; lt.samplerRow1[k] = row1[k]; }
      lt.mult = (float)power; lt.geomType = 6; lt.distType = 1; lt.texId = envTex; lt.camBackTexId = backTex;     // LIGHT_GEOM_ENV, LIGHT_DIST_OMNI
      M4 tr = m4Identity();
      for (int k = 0; k < 4; k++) { tr.m[0][k] = row0[k]; tr.m[1][k] = row1[k]; }
      const M4 ti = m4Inverse(tr);
      for (int k = 0; k < 4; k++) { lt.samplerRow0Inv[k] = (float)ti.m[0][k]; lt.samplerRow1Inv[k] = (float)ti.m[1][k]; }
      // PdfTableFromImage + PrefixSumm (integrator_pt_scene_lgt.cpp:219-270): max(r, g, b) at the texel centres, floored at a tenth of the mean
      const int tw = (int)tex.width, th = (int)tex.height;
      const float* texels = (const float*)tex.bytes.data();
      std::vector<float> lum((size_t)tw * th);
      float avg = 0.0f;
      for (int y = 0; y < th; y++) {
        float avgInRow = 0.0f;
        for (int x = 0; x < tw; x++) { const float* c4 = texels + 4 * ((size_t)y * tw + x); const float l = std::max(c4[0], std::max(c4[1], c4[2])); lum[(size_t)y * tw + x] = l; avgInRow += l; }
        avg += avgInRow;
      }
      avg /= float(tw * th);
      lt.pdfTableOffset = (uint32_t)sc.arrays1f.size(); lt.pdfTableSize = (uint32_t)lum.size() + 1u; lt.pdfTableSizeX = (uint32_t)tw; lt.pdfTableSizeY = (uint32_t)th;
      double accum = 0.0;
      for (size_t i = 0; i < lum.size(); i++) { sc.arrays1f.push_back((float)accum); accum += (double)std::max(lum[i], 0.1f * avg); }
      sc.arrays1f.push_back((float)accum);
      sc.envLightId = (uint32_t)sc.lights.size();
      oldToNew.push_back((int)sc.lights.size());
      sc.lights.push_back(lt);
      continue;
    }
    LightSource lt = blankLight();
    lightFrame(m, lt);
    for (int k = 0; k < 3; k++) lt.intensity[k] = (float)color[k];
    if (color.size() >= 4) lt.intensity[3] = (float)color[3];
    lt.specId = spectrumId(inten->child("color"));                            // LoadLightSourceFromNode (integrator_pt_scene_lgt.cpp:22-25)
    lt.mult = (float)power;
    const XmlNode* size = ln->child("size");
    if (ltype == "directional") lt.geomType = 4;
    else if (shape == "rect" || shape == "disk") {
      const double hw = size ? std::atof(size->get("half_width", "0").c_str()) : 0.0, hl = size ? std::atof(size->get("half_length", "0").c_str()) : 0.0;
      M4 rot = m; rot.m[0][3] = rot.m[1][3] = rot.m[2][3] = 0.0; rot.m[3][3] = 1.0;
      m4ToColMajor(rot, lt.matrix);
      lt.size[0] = (float)hl; lt.size[1] = (float)hw;
      const double sx = colLen(m, 0), sz = colLen(m, 2);
      if (shape == "disk") { const double r = std::atof(size->get("radius").c_str()); lt.geomType = 2; lt.size[0] = (float)r; lt.pdfA = (float)(1.0 / (M_PI * r * r * sx * sz)); }
      else { lt.geomType = 1; lt.pdfA = (float)(1.0 / (4.0 * hl * hw * sx * sz)); }
    } else if (shape == "sphere") {
      const double r = std::atof(size->get("radius").c_str()) * colLen(m, 0);
      lt.norm[0] = 0.0f; lt.norm[1] = -1.0f; lt.norm[2] = 0.0f; lt.norm[3] = 0.0f;
      lt.geomType = 3; lt.size[0] = lt.size[1] = (float)r; lt.pdfA = (float)(1.0 / (4.0 * M_PI * r * r));
    } else {
      lt.geomType = 5; lt.pdfA = 1.0f;
      lt.distType = (dist == "omni" || dist == "uniform" || dist == "ies") ? 1u : (dist == "spot" ? 2u : 0u);
      if (dist == "spot") {                                                   // integrator_pt_scene_lgt.cpp:125-160
        auto val = [](const XmlNode* n) -> float { return n ? (float)std::atof((n->has("val") ? n->get("val") : n->text).c_str()) : 0.0f; };
        const float halfRad = 0.5f * 0.017453292519943295769f;
        lt.lightCos2 = std::cos(halfRad * val(ln->child("falloff_angle")));
        lt.lightCos1 = std::cos(halfRad * val(ln->child("falloff_angle2")));
        if (const XmlNode* proj = ln->child("projective")) {                  // a slide projector: view-projection of the light in iesMatrix
          M4 rot = m; rot.m[0][3] = rot.m[1][3] = rot.m[2][3] = 0.0; rot.m[3][3] = 1.0;
          const double eye[3] = { m.m[0][3], m.m[1][3], m.m[2][3] };
          const double look[3] = { -m.m[0][1] + m.m[0][3], -m.m[1][1] + m.m[1][3], -m.m[2][1] + m.m[2][3] };     // M * (0, -1, 0, 1)
          const double up[3] = { rot.m[0][2], rot.m[1][2], rot.m[2][2] };                                         // rot * (0, 0, 1)
          const M4 vp = m4Mul(m4Perspective(val(proj->child("fov")), 1.0, val(proj->child("nearClipPlane")), val(proj->child("farClipPlane"))), m4LookAt(eye, look, up));
          m4ToColMajor(vp, lt.iesMatrix);
          if (proj->child("texture")) {
            float r0[4], r1[4]; uint32_t tid = 0;
            if (!loadTextureFromNode(proj, r0, r1, tid)) return false;
            lt.flags |= 2u; lt.texId = tid;                                   // LIGHT_FLAG_PROJECTIVE
          }
        }
      }
    }
    if (const XmlNode* ies = ln->child("ies")) {
      LoadedTexture t; if (!iesSphericalTexture(folder + "/" + ies->get("loc"), t, err)) return false;
      sc.textures.push_back(std::move(t)); lt.iesId = (uint32_t)sc.textures.size() - 1;
      if (ies->has("matrix")) {                             // mrot * transpose(transpose(matrixFromNode) * instMatrix), translation dropped
        const M4 mn = m4FromText(ies->get("matrix"));
        M4 inst = m; inst.m[0][3] = inst.m[1][3] = inst.m[2][3] = 0.0; inst.m[3][3] = 1.0;
        M4 ry = m4Identity(); const double a = M_PI / 2.0; ry.m[0][0] = std::cos(a); ry.m[0][2] = std::sin(a); ry.m[2][0] = -std::sin(a); ry.m[2][2] = std::cos(a);
        M4 im = m4Mul(ry, m4Transpose(m4Mul(m4Transpose(mn), inst)));
        im.m[0][3] = im.m[1][3] = im.m[2][3] = 0.0; im.m[3][3] = 1.0;
        m4ToColMajor(im, lt.iesMatrix);
      }
    }
    oldToNew.push_back((int)sc.lights.size());
    sc.lights.push_back(lt);
  }

  // materials: ConvertOldHydraMaterial (integrator_pt_scene_mat.cpp:280-450), every branch - emission, diffuse (+ Oren-Nayar), reflectivity
  // with and without Fresnel (coated plastic / Lambert + metal mix / pure metal), transparency (legacy glass)
  auto color4 = [](const XmlNode* n, float out[4]) {                          // GetColorFromNode (:124-143)
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    if (!n || !n->has("val")) return;
    const auto v = parseFloats(n->get("val"));
    if (v.size() == 1) out[0] = out[1] = out[2] = out[3] = (float)v[0];
    else if (v.size() == 3) { out[0] = (float)v[0]; out[1] = (float)v[1]; out[2] = (float)v[2]; }
    else if (v.size() == 4) for (int k = 0; k < 4; k++) out[k] = (float)v[k];
  };
  auto val1f = [](const XmlNode* n, float dflt = 0.0f) -> float {             // hydra_xml::readval1f (hydraxml.cpp:390-402)
    if (!n) return dflt;
    return (float)std::atof((n->has("val") ? n->get("val") : n->text).c_str());
  };
  auto len4 = [](const float* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]); };
  auto len3 = [](const float* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
  auto fdr = [](float eta) -> float {                                         // mi::fresnel_diffuse_reflectance (mi_materials.cpp:105-130)
    const float invEta = 1.0f / eta;
    const float approx1 = 0.0636f * invEta + (eta * (eta * (-1.4399f) + 0.7099f) + 0.6681f);
    const float cs[6] = { -1.36881f, 4.98554f, -7.80989f, 6.75335f, -3.4793f, 0.919317f };
    float acc = 0.0f; for (float c : cs) acc = acc * invEta + c;
    return eta < 1.0f ? approx1 : acc;
  };
  // SetMiPlastic (mi_materials.cpp:455-469)
  auto setMiPlastic = [&](Material& mat, float intIor, float extIor, const float* diffuse, const float* specular) {
    for (int k = 0; k < 4; k++) { mat.colors[0][k] = diffuse[k]; mat.colors[1][k] = specular[k]; }
    const float eta = intIor / extIor;
    mat.data[5] = eta; mat.data[0] = fdr((float)(1.0 / (double)eta)); mat.data[1] = fdr(eta);
    const double dMean = 0.3333333 * ((double)diffuse[0] + diffuse[1] + diffuse[2]), sMean = 0.3333333 * ((double)specular[0] + specular[1] + specular[2]);
    mat.data[2] = (float)(sMean / (dMean + sMean));
  };
  // LoadSceneMaterials (integrator_pt_scene.cpp:603-638): texid[1] = none, or the <displacement type="normal_bump"> map
  auto applyNormalMap = [&](const XmlNode* mn, Material& mat) -> bool {
    mat.texid[1] = 0xFFFFFFFFu;
    const XmlNode* disp = mn->child("displacement");
    if (!disp || disp->get("type") != "normal_bump") return true;            // other bump types: message only in the reference
    const XmlNode* nm = disp->child("normal_map");
    if (!loadTextureFromNode(nm, mat.row0[1], mat.row1[1], mat.texid[1])) return false;
    const XmlNode* inv = nm ? nm->child("invert") : nullptr;
    auto flag = [&](const char* name) { return inv && (int)std::atof(inv->get(name, "0").c_str()) == 1; };
    if (flag("x")) mat.cflags |= 32u;
    if (flag("y")) mat.cflags |= 64u;
    if (flag("swap_xy")) mat.cflags |= 128u;
    return true;
  };
  auto attrFloat = [](const XmlNode* n) -> float { return (n && n->has("val")) ? (float)std::atof(n->get("val").c_str()) : 0.0f; };   // as_float of a missing node is 0
  auto zeroMaterial = [](Material& mat) { std::memset(&mat, 0, sizeof(mat)); for (int k = 0; k < 4; k++) mat.spdid[k] = 0xFFFFFFFFu; };   // Material mat = {}; spectra: none (RGB mode)
  // the typed material nodes of LoadSceneMaterials (integrator_pt_scene.cpp:500-570); false with err set on failure, `known` false for other types
  auto loadTypedMaterial = [&](const XmlNode* mn, const std::string& type, Material& mat, bool& known) -> bool {
    known = true;
    zeroMaterial(mat);
    const float one4[4] = {1, 1, 1, 1};
    if (type == "gltf") {                                                     // ConvertGLTFMaterial (integrator_pt_scene_mat.cpp:176-278)
      mat.mtype = 1; uint32_t cflags = 1u | 2u; mat.data[7] = 1.0f;
      for (int k = 0; k < 4; k++) { mat.row0[k][0] = 1.0f; mat.row1[k][1] = 1.0f; }
      float ior = 1.5f, gloss = 1.0f, metal = 0.0f, base[4] = {1, 1, 1, 1};
      if (const XmlNode* cn = mn->child("color")) { color4(cn, base); if (cn->child("texture") && !loadTextureFromNode(cn, mat.row0[0], mat.row1[0], mat.texid[0])) return false; }
      const XmlNode* gn = mn->child("glossiness"); const XmlNode* rn = mn->child("roughness");
      if (gn || rn) {
        const XmlNode* n = gn ? gn : rn;
        gloss = val1f(n);
        if (!gn) cflags |= 1024u;                                             // FLAG_INVERT_GLOSINESS
        if (n->child("texture")) { if (!loadTextureFromNode(n, mat.row0[2], mat.row1[2], mat.texid[2])) return false; cflags |= 256u; }
      }
      if (const XmlNode* m2 = mn->child("metalness")) {
        metal = val1f(m2);
        if (m2->child("texture")) { if (!loadTextureFromNode(m2, mat.row0[3], mat.row1[3], mat.texid[3])) return false; cflags |= 256u; }
      }
      if (const XmlNode* n = mn->child("fresnel_ior")) ior = val1f(n);
      if (const XmlNode* n = mn->child("coat")) mat.data[7] = val1f(n);
      if (const XmlNode* pn = mn->child("glossiness_metalness_coat")) {
        metal = gloss = val1f(pn); mat.data[7] = gloss;
        if (pn->child("texture")) { if (!loadTextureFromNode(pn, mat.row0[2], mat.row1[2], mat.texid[2])) return false; cflags |= 256u | 512u; }
      }
      mat.cflags = cflags;
      for (int k = 0; k < 4; k++) mat.colors[2][k] = 1.0f;
      mat.data[3] = metal; mat.data[4] = gloss;
      setMiPlastic(mat, ior, 1.0f, base, one4);
    } else if (type == "rough_conductor") {                                   // LoadRoughConductorMaterial (:452-513), RGB mode
      for (int k = 0; k < 4; k++) mat.colors[0][k] = 1.0f;
      mat.mtype = 3; mat.lightId = 0xFFFFFFFFu;
      float au, av;
      if (const XmlNode* an = mn->child("alpha")) {
        au = av = attrFloat(an);
        if (!loadTextureFromNode(an, mat.row0[0], mat.row1[0], mat.texid[0])) return false;
        if (mat.texid[0] != 0) au = av = 1.0f;
      } else { au = attrFloat(mn->child("alpha_u")); av = attrFloat(mn->child("alpha_v")); }
      mat.data[0] = au; mat.data[1] = av; mat.data[2] = attrFloat(mn->child("eta")); mat.data[3] = attrFloat(mn->child("k"));
      mat.spdid[0] = spectrumId(mn->child("eta")); mat.spdid[1] = spectrumId(mn->child("k"));                 // (:493-497)
      if (const XmlNode* rc = mn->child("reflectance")) if (!spectral) color4(rc, mat.colors[0]);             // (read in RGB mode only, :507-510)
    } else if (type == "diffuse") {                                           // LoadDiffuseMaterial (:516-571), RGB mode
      for (int k = 0; k < 4; k++) mat.colors[0][k] = 1.0f;
      mat.mtype = 4; mat.lightId = 0xFFFFFFFFu;
      const XmlNode* bsdf = mn->child("bsdf");
      if (bsdf && bsdf->get("type") == "oren-nayar") { mat.cflags = 16u; if (const XmlNode* r = mn->child("roughness")) mat.data[0] = val1f(r); }
      if (const XmlNode* rc = mn->child("reflectance")) {
        color4(rc, mat.colors[0]); if (!loadTextureFromNode(rc, mat.row0[0], mat.row1[0], mat.texid[0])) return false; mat.spdid[0] = spectrumId(rc);
        if (spectral && !loadSpectralTextures(mat.spdid[0], rc)) return false;                                   // (:562-567)
      }
    } else if (type == "dielectric") {                                        // LoadDielectricMaterial (:574-616), RGB mode
      for (int k = 0; k < 4; k++) { mat.colors[0][k] = 1.0f; mat.colors[1][k] = 1.0f; }
      mat.mtype = 7; mat.lightId = 0xFFFFFFFFu; mat.data[0] = 1.00028f; mat.data[1] = 1.5046f;
      if (const XmlNode* n = mn->child("int_ior")) { mat.data[1] = attrFloat(n); mat.spdid[0] = spectrumId(n); }   // dispersion: an IOR spectrum (:590-595)
      if (const XmlNode* n = mn->child("ext_ior")) mat.data[0] = attrFloat(n);
      if (const XmlNode* n = mn->child("reflectance")) color4(n, mat.colors[0]);
      if (const XmlNode* n = mn->child("transmittance")) color4(n, mat.colors[1]);
    } else if (type == "plastic") {                                           // LoadPlasticMaterial (:675-757), RGB mode
      mat.mtype = 5; mat.lightId = 0xFFFFFFFFu;
      if (const XmlNode* rc = mn->child("reflectance")) { color4(rc, mat.colors[0]); if (!loadTextureFromNode(rc, mat.row0[0], mat.row1[0], mat.texid[0])) return false; }
      const float intIor = val1f(mn->child("int_ior"), 1.49f), extIor = val1f(mn->child("ext_ior"), 1.000277f);
      mat.data[1] = intIor / extIor;
      mat.data[0] = val1f(mn->child("alpha"), 0.1f);
      if (mat.data[0] == 0.0f) mat.data[0] = 1e-6f;                          // "dirty hack" (:723-727)
      if (const XmlNode* nl = mn->child("nonlinear")) mat.nonlinear = (uint32_t)std::atof((nl->has("val") ? nl->get("val") : nl->text).c_str());
      const plastic::CoatPrecomputed pre = plastic::fresnelCoatPrecompute(mat.data[0], intIor, extIor, mat.colors[0], one4);
      mat.data[3] = pre.internalReflectance; mat.data[2] = pre.specularSamplingWeight;
      mat.spdid[0] = spectrumId(mn->child("reflectance"));                    // (:704-705)
      if (spectral && !loadSpectralTextures(mat.spdid[0], mn->child("reflectance"))) return false;   // (:708-713)
      if (spectral) {
        // mi::fresnel_coat_precompute in spectral mode (mi_materials.cpp:383-404): s_mean = 1 over four components, d_mean = the mean of the
        // reflectance spectrum (mi::spectrum_mean: trapezoid rule over 360 .. 830 nm in double), 0.5 without one
        float dMean = 0.5f;
        const uint32_t sid = mat.spdid[0];
        if (sid != 0xFFFFFFFFu && 2 * (size_t)sid + 1 < sc.specOffsetSz.size() && sc.specOffsetSz[2 * sid] != 0xFFFFFFFFu) {
          const float* v = sc.specValues.data() + sc.specOffsetSz[2 * sid]; const size_t n = sc.specOffsetSz[2 * sid + 1];
          const double interval = (double(kLambdaMax) - double(kLambdaMin)) / double(n - 1);
          double integral = 0.0;
          for (size_t i = 0; i + 1 < n; i++) integral += 0.5 * interval * ((double)v[i] + (double)v[i + 1]);
          dMean = float(integral) / (kLambdaMax - kLambdaMin);
        }
        mat.data[2] = 1.0f / (dMean + 1.0f);
      }
      mat.datai[0] = (uint32_t)sc.arrays1f.size();
      sc.arrays1f.insert(sc.arrays1f.end(), pre.transmittance, pre.transmittance + plastic::TRANSMITTANCE_RES);
    } else if (type == "thin_film") {                                         // LoadThinFilmMaterial (:1020-1193)
      auto fbits = [](uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; };
      mat.mtype = 8; mat.lightId = 0xFFFFFFFFu;
      mat.colors[0][0] = mat.colors[0][1] = mat.colors[0][2] = 1.0f; mat.colors[0][3] = 0.0f;
      float au, av;
      if (const XmlNode* an = mn->child("alpha")) {
        au = av = attrFloat(an);
        if (!loadTextureFromNode(an, mat.row0[0], mat.row1[0], mat.texid[0])) return false;
        if (mat.texid[0] != 0) au = av = 1.0f;
      } else { au = attrFloat(mn->child("alpha_u")); av = attrFloat(mn->child("alpha_v")); }
      mat.data[0] = au; mat.data[1] = av;                                     // FILM_ROUGH_U, FILM_ROUGH_V
      const XmlNode* tmapNode = mn->child("thickness_map");
      if (tmapNode) {
        mat.data[10] = (float)std::atof(tmapNode->get("min", "0").c_str()); mat.data[11] = (float)std::atof(tmapNode->get("max", "0").c_str());
        if (!loadTextureFromNode(tmapNode, mat.row0[2], mat.row1[2], mat.texid[2])) return false;
      }
      mat.data[12] = fbits(tmapNode ? 1u : 0u);                               // FILM_THICKNESS_MAP
      mat.data[8] = mn->child("ext_ior") ? attrFloat(mn->child("ext_ior")) : 1.00028f;   // FILM_ETA_EXT: air
      const uint32_t tOff = (uint32_t)sc.filmsThickness.size(), sOff = (uint32_t)sc.filmsSpecId.size(), eOff = (uint32_t)sc.filmsEtaK.size();
      mat.data[9] = fbits(tOff); mat.data[6] = fbits(sOff); mat.data[4] = fbits(eOff);   // FILM_THICKNESS_OFFSET, FILM_ETA_SPECID_OFFSET, FILM_ETA_OFFSET
      std::vector<const XmlNode*> stack;                                      // the <layers> children, then the material's own <eta> / <k> (the substrate)
      if (const XmlNode* ln = mn->child("layers")) for (const XmlNode& l : ln->children) stack.push_back(&l);
      for (const XmlNode* l : stack) if (const XmlNode* t = l->child("thickness")) sc.filmsThickness.push_back(attrFloat(t));
      if (mn->child("eta")) stack.push_back(mn);
      const uint32_t layers = (uint32_t)stack.size();
      if (layers < 1 || layers > film::MAX_LAYERS || sc.filmsThickness.size() <= tOff) { err = "thin_film material without layers or without a thickness"; return false; }
      for (const XmlNode* l : stack) { sc.filmsEtaK.push_back(attrFloat(l->child("eta"))); sc.filmsSpecId.push_back(spectrumId(l->child("eta"))); }
      mat.data[13] = sc.filmsThickness[tOff]; mat.data[14] = fbits(layers);   // FILM_THICKNESS, FILM_LAYERS_COUNT
      mat.data[7] = fbits((uint32_t)sc.filmsSpecId.size()); mat.data[5] = fbits((uint32_t)sc.filmsEtaK.size());   // FILM_K_SPECID_OFFSET, FILM_K_OFFSET
      for (const XmlNode* l : stack) { sc.filmsEtaK.push_back(attrFloat(l->child("k"))); sc.filmsSpecId.push_back(spectrumId(l->child("k"))); }
      uint32_t transpar = 0;
      if (const XmlNode* tn = mn->child("transparent")) transpar = (uint32_t)std::atoll(tn->get("val", "0").c_str());
      mat.data[15] = fbits(transpar);                                         // FILM_TRANSPARENT
      film::Params fp;
      fp.spectralMode = spectral ? 1 : 0; fp.extIOR = mat.data[8]; fp.layers = layers;
      fp.eta = sc.filmsEtaK.data() + eOff; fp.k = sc.filmsEtaK.data() + eOff + layers; fp.etaSpecId = sc.filmsSpecId.data() + sOff; fp.kSpecId = sc.filmsSpecId.data() + sOff + layers;
      fp.thickness = sc.filmsThickness.data() + tOff; fp.thicknessMap = tmapNode ? 1 : 0; fp.thicknessMin = mat.data[10]; fp.thicknessMax = mat.data[11];
      fp.specValues = sc.specValues.empty() ? nullptr : sc.specValues.data(); fp.specOffsetSz = sc.specOffsetSz.data(); fp.numSpectra = (uint32_t)(sc.specOffsetSz.size() / 2);
      fp.cieXYZ = sc.cieXYZ.data();
      const bool pre = film::precomputed(fp);
      mat.data[2] = fbits(pre ? 1u : 0u); mat.data[3] = fbits(pre ? (uint32_t)sc.precompThinFilms.size() : 0u);   // FILM_PRECOMP_FLAG, FILM_PRECOMP_OFFSET
      if (pre) {
        const size_t at = sc.precompThinFilms.size();
        sc.precompThinFilms.resize(at + film::tableSize(fp));
        if (!film::precompute(fp, sc.precompThinFilms.data() + at)) { err = "thin_film material: the tables could not be computed"; return false; }
      }
    } else if (type == "blend") {                                             // LoadBlendMaterial (:619-647)
      mat.mtype = 6; mat.data[0] = 1.0f;
      if (const XmlNode* n = mn->child("bsdf_1")) mat.datai[0] = (uint32_t)std::atoll(n->get("id", "0").c_str());
      if (const XmlNode* n = mn->child("bsdf_2")) mat.datai[1] = (uint32_t)std::atoll(n->get("id", "0").c_str());
      if (const XmlNode* wn = mn->child("weight")) { mat.data[0] = val1f(wn); if (!loadTextureFromNode(wn, mat.row0[0], mat.row1[0], mat.texid[0])) return false; }
    } else known = false;
    return true;
  };
  if (const XmlNode* lib = root.child("materials_lib")) for (const XmlNode* mn : lib->all("material")) {
    Material mat; std::memset(&mat, 0, sizeof(mat));
    const std::string mtypeAttr = mn->get("type");
    if (mtypeAttr != "hydra_material") {
      bool known = false;
      if (!loadTypedMaterial(mn, mtypeAttr, mat, known)) return false;
      if (!known) { err = "xml: material type '" + mtypeAttr + "' is not one of the reference's"; return false; }
      for (int k = 0; k < 4; k++) {
        bool zero = true; for (int j = 0; j < 4; j++) zero = zero && mat.row0[k][j] == 0.0f && mat.row1[k][j] == 0.0f;
        if (zero) { mat.row0[k][0] = 1.0f; mat.row1[k][1] = 1.0f; }
      }
      if (!applyNormalMap(mn, mat)) return false;
      const int lid = mn->has("light_id") ? std::atoi(mn->get("light_id").c_str()) : -1;
      if (lid >= 0 && lid < (int)sc.lights.size()) {
        for (int k = 0; k < 4; k++) mat.colors[0][k] = sc.lights[(size_t)lid].intensity[k];
        mat.data[0] = sc.lights[(size_t)lid].mult;
        mat.spdid[0] = sc.lights[(size_t)lid].specId;
        sc.lights[(size_t)lid].matId = (uint32_t)sc.materials.size();
      }
      sc.materials.push_back(mat);
      continue;
    }
    mat.mtype = 1; mat.data[3] = 0.0f; mat.data[7] = 1.0f;                    // MAT_TYPE_GLTF, GLTF_FLOAT_ALPHA, GLTF_FLOAT_REFL_COAT
    for (int k = 0; k < 4; k++) { mat.colors[1][k] = 1.0f; mat.colors[2][k] = 0.0f; }   // GLTF_COLOR_COAT, GLTF_COLOR_METAL
    mat.lightId = 0xFFFFFFFFu;
    const XmlNode* emis = mn->child("emission");
    float color[4] = {0, 0, 0, 0};
    bool isEmission = false;
    if (mn->has("light_id") || emis) {
      const XmlNode* cn = emis ? emis->child("color") : nullptr;
      color4(cn, color);
      isEmission = mn->has("light_id") || len4(color) > 1e-5f;
      if (!loadTextureFromNode(cn, mat.row0[0], mat.row1[0], mat.texid[0])) return false;
      for (int k = 0; k < 4; k++) mat.colors[0][k] = color[k];
      mat.lightId = mn->has("light_id") ? (uint32_t)std::atoi(mn->get("light_id").c_str()) : 0xFFFFFFFFu;
      mat.spdid[0] = spectrumId(cn);                                          // GetSpectrumIdFromNode(nodeEmissColor) (:319-320)
      mat.mtype = 0xEFFFFFFFu;
      const XmlNode* mult = cn ? cn->child("multiplier") : nullptr;
      mat.data[0] = mult ? val1f(mult) : 1.0f;
    }
    const XmlNode* diff = mn->child("diffuse");
    const XmlNode* dn = diff ? diff->child("color") : nullptr;
    if (dn) {
      color4(dn, color);
      if (dn->child("texture")) { if (!loadTextureFromNode(dn, mat.row0[0], mat.row1[0], mat.texid[0])) return false; }
    }
    float reflColor[4] = {0, 0, 0, 0}, reflGloss = 1.0f, fresnelIOR = 1.5f;
    const XmlNode* refl = mn->child("reflectivity");
    if (refl) { color4(refl->child("color"), reflColor); reflGloss = val1f(refl->child("glossiness")); fresnelIOR = val1f(refl->child("fresnel_ior")); }
    float transpColor[4] = {0, 0, 0, 0}, transpGloss = 1.0f;
    if (const XmlNode* tr = mn->child("transparency")) { color4(tr->child("color"), transpColor); transpGloss = val1f(tr->child("glossiness")); }
    const XmlNode* fres = refl ? refl->child("fresnel") : nullptr;
    const bool hasFresnel = fres && (int)std::atof(fres->get("val", "0").c_str()) != 0;
    if (!hasFresnel) fresnelIOR = 0.0f;
    auto set4 = [](float* d, const float* v) { for (int k = 0; k < 4; k++) d[k] = v[k]; };
    auto fill4 = [](float* d, float v) { for (int k = 0; k < 4; k++) d[k] = v; };
    if ((len4(reflColor) > 1e-5f && len3(color) > 1e-5f) || hasFresnel) {
      mat.mtype = 1; mat.lightId = 0xFFFFFFFFu;
      set4(mat.colors[0], color); set4(mat.colors[1], reflColor);
      if (hasFresnel) {
        mat.data[3] = 0.0f; mat.data[7] = 1.0f; fill4(mat.colors[2], 0.0f); mat.cflags = 1u | 2u;
        // SetMiPlastic(&mat, fresnelIOR, 1.0f, color, reflColor) (mi_materials.cpp:455-469)
        const float eta = fresnelIOR / 1.0f;
        mat.data[5] = eta; mat.data[0] = fdr((float)(1.0 / (double)eta)); mat.data[1] = fdr(eta);
        const double dMean = 0.3333333 * ((double)color[0] + color[1] + color[2]), sMean = 0.3333333 * ((double)reflColor[0] + reflColor[1] + reflColor[2]);
        mat.data[2] = (float)(sMean / (dMean + sMean));
      } else {
        mat.data[3] = len4(reflColor) / (len4(reflColor) + len3(color)); mat.data[7] = 0.0f;
        fill4(mat.colors[1], 0.0f); set4(mat.colors[2], reflColor); mat.cflags = 1u | 4u;
      }
    } else if (len4(reflColor) > 1e-5f) {
      mat.mtype = 1; mat.cflags = 4u; set4(mat.colors[0], reflColor); fill4(mat.colors[2], 1.0f); fill4(mat.colors[1], 0.0f); mat.data[3] = 1.0f;
    } else if (len3(color) > 1e-5f) {
      mat.mtype = 1; mat.cflags = 1u; set4(mat.colors[0], color); fill4(mat.colors[1], 0.0f); fill4(mat.colors[2], 0.0f); mat.data[3] = 0.0f; mat.data[7] = 0.0f;
    }
    if (len4(transpColor) > 1e-5f) {                                          // legacy glass (MAT_TYPE_GLASS = 2)
      mat.mtype = 2; set4(mat.colors[0], reflColor); set4(mat.colors[1], transpColor);
      mat.data[0] = reflGloss; mat.data[1] = transpGloss; mat.data[2] = fresnelIOR;
    }
    if (isEmission) mat.mtype = 0xEFFFFFFFu;
    if (const XmlNode* r = diff ? diff->child("roughness") : nullptr) { mat.data[6] = val1f(r); mat.cflags |= 16u; }   // Oren-Nayar
    mat.data[4] = reflGloss; mat.data[5] = fresnelIOR;
    for (int k = 0; k < 4; k++) {                                             // unused texture slots: identity rows, no normal map (integrator_pt_scene.cpp:600-608)
      bool zero = true; for (int j = 0; j < 4; j++) zero = zero && mat.row0[k][j] == 0.0f && mat.row1[k][j] == 0.0f;
      if (zero) { mat.row0[k][0] = 1.0f; mat.row1[k][1] = 1.0f; }
    }
    if (!applyNormalMap(mn, mat)) return false;
    if (mat.mtype == 0xEFFFFFFFu) {
      const int lid = mn->has("light_id") ? std::atoi(mn->get("light_id").c_str()) : -1;
      if (lid >= 0 && lid < (int)sc.lights.size()) {                          // LoadScene :973-996: the light's intensity wins
        for (int k = 0; k < 4; k++) mat.colors[0][k] = sc.lights[(size_t)lid].intensity[k];
        mat.data[0] = sc.lights[(size_t)lid].mult;
        sc.lights[(size_t)lid].matId = (uint32_t)sc.materials.size();
      }
    }
    sc.materials.push_back(mat);
  }

  // geometry: cmesh4::LoadMeshFromVSGF; m_vData8f packs {normal.xyz, u | tangent.xyz, v} (integrator_pt_scene.cpp:727-837)
  if (const XmlNode* lib = root.child("geometry_lib")) for (const XmlNode* mesh : lib->all("mesh")) {
    if (mesh->get("ptrs") == "1") {                                            // LoadSceneGeometry's pointer branch (integrator_pt_scene.cpp:750-789)
      const int meshId = std::atoi(mesh->get("id").c_str());
      const auto it = meshPtrs ? meshPtrs->find(meshId) : std::unordered_map<int, Mesh4fInput>::const_iterator();
      if (!meshPtrs || it == meshPtrs->end()) { err = "[LoadSceneGeometry]: bad mesh pointer id = " + std::to_string(meshId); return false; }
      const Mesh4fInput& in = it->second;
      if (!in.vPosPtr || !in.vNormPtr4f || !in.vTexCoord2f || !in.indicesPtr || in.vPosByteStride % 4 != 0 || in.vPosByteStride < 12) { err = "[LoadSceneGeometry]: incomplete mesh pointers, id = " + std::to_string(meshId); return false; }
      const uint32_t nv = in.vertNum, nt = in.indicesNum / 3, fs = in.vPosByteStride / 4;
      sc.matVertOffset.push_back((uint32_t)sc.matIdByPrimId.size()); sc.matVertOffset.push_back((uint32_t)(sc.vPos4f.size() / 4));
      sc.geomTriCount.push_back(nt); sc.geomVertCount.push_back(nv);
      for (uint32_t v = 0; v < nv; v++) {
        const float* pp = in.vPosPtr + (size_t)fs * v;
        const float p4[4] = { pp[0], pp[1], pp[2], fs >= 4 ? pp[3] : 1.0f };
        sc.vPos4f.insert(sc.vPos4f.end(), p4, p4 + 4);
        float d[8] = { in.vNormPtr4f[4 * v], in.vNormPtr4f[4 * v + 1], in.vNormPtr4f[4 * v + 2], in.vTexCoord2f[2 * v], 0, 0, 0, in.vTexCoord2f[2 * v + 1] };
        if (in.vTangPtr4f) { d[4] = in.vTangPtr4f[4 * v]; d[5] = in.vTangPtr4f[4 * v + 1]; d[6] = in.vTangPtr4f[4 * v + 2]; }   // (else: "render must not compute tangent space")
        sc.vData8f.insert(sc.vData8f.end(), d, d + 8);
      }
      sc.triIndices.insert(sc.triIndices.end(), in.indicesPtr, in.indicesPtr + (size_t)nt * 3);
      if (in.matIdNum != nt || !in.matIdPtr) sc.matIdByPrimId.insert(sc.matIdByPrimId.end(), nt, in.matIdAll);
      else sc.matIdByPrimId.insert(sc.matIdByPrimId.end(), in.matIdPtr, in.matIdPtr + nt);
      continue;
    }
    std::vector<uint8_t> f; const std::string p = folder + "/" + mesh->get("loc");
    if (!readFile(p, f) || f.size() < 24) { err = "cannot read " + p; return false; }
    uint32_t nv, ni, nm, flags; std::memcpy(&nv, f.data() + 8, 4); std::memcpy(&ni, f.data() + 12, 4); std::memcpy(&nm, f.data() + 16, 4); std::memcpy(&flags, f.data() + 20, 4);
    size_t off = 24;
    const size_t need = 24 + (size_t)nv * 16 * (1 + ((flags & 8u) ? 0 : 1) + ((flags & 1u) ? 1 : 0)) + (size_t)nv * 8 + (size_t)ni * 4 + (size_t)(ni / 3) * 4;
    if (f.size() < need) { err = "vsgf truncated: " + p; return false; }
    const float* pos = (const float*)(f.data() + off); off += (size_t)nv * 16;
    const float* norm = nullptr; if (!(flags & 8u)) { norm = (const float*)(f.data() + off); off += (size_t)nv * 16; }
    const float* tang = nullptr; if (flags & 1u) { tang = (const float*)(f.data() + off); off += (size_t)nv * 16; }
    const float* uv = (const float*)(f.data() + off); off += (size_t)nv * 8;
    const uint32_t* idx = (const uint32_t*)(f.data() + off); off += (size_t)ni * 4;
    const uint32_t* mats = (const uint32_t*)(f.data() + off);
    const uint32_t nt = ni / 3;
    sc.matVertOffset.push_back((uint32_t)sc.matIdByPrimId.size()); sc.matVertOffset.push_back((uint32_t)(sc.vPos4f.size() / 4));
    sc.geomTriCount.push_back(nt); sc.geomVertCount.push_back(nv);
    sc.vPos4f.insert(sc.vPos4f.end(), pos, pos + (size_t)nv * 4);
    for (uint32_t v = 0; v < nv; v++) {
      float d[8] = { 0, 0, 0, uv[2 * v], 0, 0, 0, uv[2 * v + 1] };
      if (norm) { d[0] = norm[4 * v]; d[1] = norm[4 * v + 1]; d[2] = norm[4 * v + 2]; }
      if (tang) { d[4] = tang[4 * v]; d[5] = tang[4 * v + 1]; d[6] = tang[4 * v + 2]; }
      sc.vData8f.insert(sc.vData8f.end(), d, d + 8);
    }
    sc.triIndices.insert(sc.triIndices.end(), idx, idx + (size_t)nt * 3);
    sc.matIdByPrimId.insert(sc.matIdByPrimId.end(), mats, mats + nt);
  }

  // remap lists (hydraxml.h:267-276, LoadSceneRemapLists integrator_pt_scene.cpp:909-924): the lists back to back, then one offset per list
  // and the total size
  if (const XmlNode* rl = sceneNode->child("remap_lists")) {
    std::vector<int32_t> flat, offs;
    for (const XmlNode& nodeRef : rl->children) {
      const XmlNode* node = &nodeRef;
      const int n = std::atoi(node->get("size", "0").c_str());
      const auto vals = parseFloats(node->get("val"));
      offs.push_back((int32_t)flat.size());
      for (int i = 0; i < n; i++) flat.push_back(i < (int)vals.size() ? (int32_t)vals[(size_t)i] : 0);
    }
    offs.push_back((int32_t)flat.size());
    sc.allRemapListsSize = (uint32_t)flat.size();
    sc.allRemapLists = flat; sc.allRemapLists.insert(sc.allRemapLists.end(), offs.begin(), offs.end());
  }

  // instances: matrix, m_normMatrices = transpose(inverse4x4(M)) (integrator_pt_scene.cpp:852-885), remap list and light ids
  std::vector<M4> endMatrices;                                                // the matrix at the end of the motion, per instance
  for (const XmlNode* inst : sceneNode->all("instance")) {
    const M4 m = m4FromText(inst->get("matrix"));
    float cm[16]; m4ToColMajor(m, cm); sc.instMatrices.insert(sc.instMatrices.end(), cm, cm + 16);
    m4ToColMajor(m4Transpose(m4Inverse(m)), cm); sc.normMatrices.insert(sc.normMatrices.end(), cm, cm + 16);
    const XmlNode* mot = inst->child("motion");                              // hydraxml.h:170-176
    const M4 m1 = mot ? m4FromText(mot->get("matrix")) : m;
    endMatrices.push_back(m1);
    m4ToColMajor(m1, cm); sc.instMatricesMotion.insert(sc.instMatricesMotion.end(), cm, cm + 16);
    sc.instHasMotion.push_back(mot ? 1u : 0u);
    sc.instGeomId.push_back((uint32_t)std::atoi(inst->get("mesh_id").c_str()));
    int lightId = -1;
    if (inst->has("linst_id")) { const int li = std::atoi(inst->get("linst_id").c_str()); if (li >= 0 && li < (int)oldToNew.size()) lightId = oldToNew[(size_t)li]; }
    sc.remapInst.push_back(inst->has("rmap_id") ? std::atoi(inst->get("rmap_id").c_str()) : -1);
    sc.remapInst.push_back(lightId);
  }
  bool anyMotion = false; for (uint32_t f : sc.instHasMotion) anyMotion = anyMotion || f != 0;
  if (anyMotion) {                                                           // m_normMatrices2 appended, m_normMatrices2Offs = the instance count (:888-897)
    const size_t ni = sc.instGeomId.size();
    sc.normMatrices2Offs = (uint32_t)ni;
    for (size_t i = 0; i < ni; i++) {
      float cm[16]; m4ToColMajor(m4Transpose(m4Inverse(endMatrices[i])), cm); sc.normMatrices.insert(sc.normMatrices.end(), cm, cm + 16);
    }
  }
  return true;
}

} // namespace hydra_hip
