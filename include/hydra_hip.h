/* hydra_hip.h -- C ABI of the MI355X-native (gfx950) path-tracing core.
 *
 * This is the whole drop-in boundary: plain pointers and sizes, no C++ types, no torch types. A host adapter
 * (hydracore3_amd/csrc/integrator_hip.h: class IntegratorHIP, class BVH2SceneHIP) exposes it through the
 * reference's own class surface; INTEGRATION.md shows the subclass a HydraCore3 maintainer would add.
 *
 * Every entry point names the reference interface it replaces (paths relative to the HydraCore3 tree).
 * All functions return 0 on success and a non-zero code on failure unless stated otherwise;
 * hpt_last_error() gives the message. Nothing throws across this boundary. One hpt_ctx per GPU; all calls
 * on a context come from one host thread (as in the reference: main.cpp, drmain.cpp).
 */
#ifndef HYDRA_HIP_H
#define HYDRA_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPT_OK            0
#define HPT_ERR_ARG       1   /* bad argument (the reference prints and returns, e.g. EmbreeRT.cpp:144-159) */
#define HPT_ERR_HIP       2   /* HIP runtime error */
#define HPT_ERR_STATE     3   /* call order violated (e.g. render before CommitDeviceData) */
#define HPT_ERR_UNSUPPORTED 4 /* scene uses a feature outside the hot path's scope */
#define HPT_ERR_NOMEM     5   /* a host allocation failed (std::bad_alloc / std::length_error caught at the boundary: sizes no host can hold) */

typedef struct hpt_ctx hpt_ctx;

/* texture + sampler: LiteImage::ICombinedImageSampler (integrator_pt.h:577, integrator_pt_scene_tex.cpp:19-103) */
typedef struct hpt_texture_desc {
  uint32_t width, height;
  uint32_t format;    /* 0: RGBA8 in a uint32 (r = low byte), 1: RGBA32F, 2: R32F */
  uint32_t flags;     /* bit 0: sRGB decode (rgb^2.2 after filtering; HydraSampler::inputGamma, integrator_pt.h:71) */
  uint32_t addressU;  /* LiteImage::Sampler::AddressMode: 0 WRAP, 2 CLAMP */
  uint32_t addressV;
  uint32_t filter;    /* LiteImage::Sampler::Filter: 0 NEAREST, 1 LINEAR */
  uint32_t reserved;
  const void* data;   /* host pointer, row-major, row 0 first */
} hpt_texture_desc;

/* The flat scene vectors Integrator::LoadScene fills (integrator_pt.h:472-500), as {pointer,count} pairs. */
typedef struct hpt_scene_desc {
  uint32_t numGeoms, numInsts, numVerts, numTris;
  const float*    vPos4f;         /* float4 x numVerts: positions handed to AddGeom_Triangles3f (integrator_pt_scene.cpp:799-800) */
  const float*    vData8f;        /* m_vData8f: {norm.xyz, u | tang.xyz, v} x numVerts (integrator_pt.h:479-484) */
  const uint32_t* triIndices;     /* m_triIndices: 3 x numTris, mesh-local */
  const uint32_t* matIdByPrimId;  /* m_matIdByPrimId: numTris */
  const uint32_t* matVertOffset;  /* m_matVertOffset: uint2 x numGeoms (triOffset, vertOffset) */
  const uint32_t* geomTriCount;   /* numGeoms */
  const uint32_t* geomVertCount;  /* numGeoms */
  const uint32_t* instGeomId;     /* numInsts: geomId passed to AddInstance, in instance order (integrator_pt_scene.cpp:852-885) */
  const float*    instMatrices;   /* numInsts column-major float4x4 (CrossRT.h:134, EmbreeRT.cpp:256) */
  const float*    normMatrices;   /* m_normMatrices: numInsts column-major float4x4 (integrator_pt_scene.cpp:877) */
  const int32_t*  remapInst;      /* m_remapInst: int2 x numInsts (remap list id, light id) */
  const int32_t*  allRemapLists;  /* m_allRemapLists: lists then offsets (integrator_pt_scene.cpp:909-924) */
  uint32_t        allRemapListsLen;
  uint32_t        allRemapListsSize; /* m_allRemapListsSize */
  const void*     materials;      /* m_materials: 320-byte Material records (include/cmaterial.h:187-203) */
  uint32_t        numMaterials;
  uint32_t        numLights;
  const void*     lights;         /* m_lights: 320-byte LightSource records (include/clight.h:19-56) */
  const hpt_texture_desc* textures; /* m_textures */
  uint32_t        numTextures;
  uint32_t        numArrays1f;
  const float*    arrays1f;       /* m_arrays1f: the environment light's pdf table (integrator_pt_scene.cpp:464-475); may be NULL */
  /* motion blur (integrator_pt_scene.cpp:848-897): with normMatrices2Offs != 0 (= numInsts) normMatrices holds 2 x numInsts matrices, the
   * second half for the end of the motion; instMatricesMotion / instHasMotion are read only when the geometry comes with the tables
   * (vPos4f != NULL) and stand for AddInstanceMotion(geomId, {matrix, matrix_motion}, 2) (:864-868). All may be NULL / 0. */
  const float*    instMatricesMotion; /* numInsts column-major float4x4: the instance matrix at time 1 */
  const uint32_t* instHasMotion;      /* numInsts flags */
  uint32_t        normMatrices2Offs;  /* m_normMatrices2Offs */
  uint32_t        reserved;
  /* spectral rendering (integrator_pt.h: m_spec_values, m_spec_offset_sz, m_cie_xyz, m_camResponseSpectrumId / m_camResponseType): all may be
   * NULL / 0 for RGB rendering. specValues: every spectrum resampled at 1 nm from LAMBDA_MIN = 360 (Spectrum::ResampleUniform, 471 floats each);
   * specOffsetSz: uint2 {offset, size} per spectrum id (0xFFFFFFFF offset: a spectrum given by textures, see specTexOffsetSz below);
   * cieXYZ: float4 {x, y, z, 0} x 471, the CIE 1931 observer at 360..830 nm (LoadScene fills it from Get_CIE_X/Y/Z, integrator_pt_scene.cpp:962-969). */
  const float*    specValues;
  const uint32_t* specOffsetSz;
  uint32_t        numSpecValues, numSpectra;
  const float*    cieXYZ;
  uint32_t        numCieXYZ;
  int32_t         camResponseSpectrumId[3];   /* -1: none (then SpectrumToXYZ + XYZToRGB) */
  uint32_t        camResponseType;            /* m_camResponseType: 0 = CAM_RESPONCE_XYZ, 1 = CAM_RESPONCE_RGB (integrator_pt.h:531-534) */
  uint32_t        reserved2;
  /* thin films (MAT_TYPE_THIN_FILM, integrator_pt.h:587-590): m_films_thickness_vec, m_films_spec_id_vec, m_films_eta_k_vec and the loader's
   * reflectance / transmittance tables m_precomp_thin_films (LoadThinFilmMaterial, integrator_pt_scene_mat.cpp:1020-1193; hpt_film_precompute
   * computes one material's). All may be NULL / 0 for scenes without films. */
  const float*    filmsThickness;
  const uint32_t* filmsSpecId;
  const float*    filmsEtaK;
  const float*    precompThinFilms;
  uint32_t        numFilmsThickness, numFilmsSpecId, numFilmsEtaK, numPrecompThinFilms;
  /* spectra given by textures (KSPEC_SPD_TEX; LoadSceneSpectrumData, integrator_pt_scene.cpp:363-377): m_spec_tex_ids_wavelengths = uint2 {texture,
   * wavelength in nm} per band, m_spec_tex_offset_sz = uint2 {first band, bands} per spectrum id ({0xFFFFFFFF, 0}: a tabulated spectrum). NULL / 0
   * without such spectra. */
  const uint32_t* specTexIdsWavelengths;
  const uint32_t* specTexOffsetSz;
  uint32_t        numSpecTexBands, reserved3;
} hpt_scene_desc;

/* The plain-data members UpdateMembersPlainData() refreshes before every *Block call (integrator_pt.h:268, main.cpp:398). */
typedef struct hpt_params {
  float    projInv[16];       /* m_projInv, column-major */
  float    worldViewInv[16];  /* m_worldViewInv */
  int32_t  winStartX, winStartY, winWidth, winHeight, fbWidth, fbHeight; /* SetViewport / SetFrameBufferSize (integrator_pt.h:365-392) */
  uint32_t traceDepth;        /* m_traceDepth */
  uint32_t integratorType;    /* m_intergatorType: 0 naive, 1 shadow, 2 MIS (integrator_pt.h:330-332) */
  uint32_t renderLayer;       /* m_renderLayer: FB_COLOR / FB_DIRECT / FB_INDIRECT (integrator_pt.h:406-408) */
  uint32_t tileSize;          /* m_tileSize */
  uint32_t spectralMode;      /* m_spectral_mode: 0 = RGB; 1 = four wavelengths per path (needs hpt_scene_desc's spectral tables; PathTraceBlock, NaivePathTraceBlock and
                               * PathTraceFromInputRaysBlock, every material / light / camera feature of the RGB path; channels: 1, 3 - 4, or more = wavelength layers;
                               * PathTraceDR is refused with HPT_ERR_UNSUPPORTED) */
  uint32_t envSpecIdPlus1;    /* m_envSpecId + 1 (integrator_pt.h:524; 0 = none, so that a zeroed struct means "no environment spectrum") */
  float    exposureMult, camLensRadius, camTargetDist, envSpecMult;   /* envSpecMult: m_envSpecMult (spectral mode: the environment spectrum's multiplier) */
  float    camRespoceRGB[4];  /* m_camRespoceRGB */
  float    envColor[4];       /* m_envColor */
  /* the environment of LoadSceneLights (integrator_pt_scene.cpp:441-478), read by EnvironmentColor / kernel_HitEnvironment
   * (integrator_pt_lgt.cpp:175-210, integrator_pt.cpp:550-595): 0xFFFFFFFF = none */
  uint32_t envTexId;          /* m_envTexId: index into the texture table */
  uint32_t envLightId;        /* m_envLightId: the LIGHT_GEOM_ENV entry of m_lights when the map is sampled explicitly */
  uint32_t envCamBackId;      /* m_envCamBackId: texture shown to primary rays that miss */
  uint32_t envEnableSam;      /* m_envEnableSam */
  float    envSamRow0[4], envSamRow1[4]; /* m_envSamRow0 / m_envSamRow1 */
} hpt_params;

/* CRT_Hit (external/CrossRT/CrossRT.h:23-30) */
typedef struct hpt_hit {
  float t; uint32_t primId, instId, geomId; float coords[4];
} hpt_hit;

/* ---- lifetime ------------------------------------------------------------------------------------------------- */
int  hpt_create(int device, hpt_ctx** out);          /* Integrator::Integrator + CreateSceneRT (integrator_pt.h:127-137, CrossRT.h:195) */
void hpt_destroy(hpt_ctx* ctx);                      /* Integrator::~Integrator + DeleteSceneRT (CrossRT.h:196) */
const char* hpt_last_error(hpt_ctx* ctx);
int  hpt_device_info(hpt_ctx* ctx, int* numCUs, int* wavefront, char* name, size_t nameLen);
/* Device memory for callers of the *_dev entry points that do not link the HIP runtime themselves (a plain C/C++ host such as
 * diff_render/drmain.cpp:174-261 keeping its texture, gradient and Adam moments resident). No reference counterpart: the reference's
 * generated GPU class owns its buffers (main.cpp:221-224). kind: 1 host->device, 2 device->host, 3 device->device; copies are
 * synchronous, memset is asynchronous on the null stream. */
/* Integrator::SetLines + SetPhysSize with m_enableOpticSim (integrator_pt.h:353-362; LoadOpticsFromNode integrator_pt_scene.cpp:1078-1141): the
 * lens stack traced from the film by SampleCameraRay (integrator_pt.cpp:79-103, 806-938). lines4 = n x {curvatureRadius, thickness, eta,
 * apertureRadius}, film side first (radius 0 = the aperture stop); n = 0 switches the simulation off. Takes effect at the next call. */
int  hpt_set_optics(hpt_ctx* ctx, const float* lines4, uint32_t n, float physSizeX, float physSizeY);
/* precomputeThinFilmSpectral / precomputeThinFilmRGB (integrator_pt_scene_mat.cpp:791-1018), what LoadThinFilmMaterial (:1020-1193) appends to
 * m_precomp_thin_films for one MAT_TYPE_THIN_FILM: reflectance / transmittance from outside and from inside over wavelength x angle (spectral
 * mode) or [thickness x] angle x rgb (RGB mode). layers = the films plus the substrate (FILM_LAYERS_COUNT); eta / k / their spectrum ids per
 * layer, thickness per film; cieXYZ (float4 x 471) is read in RGB mode only. outTable == NULL asks for the size; *outPrecomputed = 0 when the
 * reference's loader would not precompute (spectral mode, one film with a thickness map: FILM_PRECOMP_FLAG stays 0). Host code; no context. */
typedef struct hpt_film_params {
  int32_t  spectralMode; float extIOR; uint32_t layers; int32_t thicknessMap;
  float    thicknessMin, thicknessMax; uint32_t numSpectra, reserved;
  const float* eta; const float* k; const uint32_t* etaSpecId; const uint32_t* kSpecId; const float* thickness;
  const float* specValues; const uint32_t* specOffsetSz; const float* cieXYZ;
} hpt_film_params;
int  hpt_film_precompute(const hpt_film_params* params, float* outTable, uint64_t outCapacity, uint64_t* outCount, int* outPrecomputed);
/* The JPEG reader of the fixture loaders (LoadTextureAndMakeCombined reads ".jpg" / ".jpeg" through LiteImage, integrator_pt_scene_tex.cpp:24-33):
 * 8-bit baseline / progressive Huffman JPEG, grey or YCbCr, to RGBA8 rows in file order (csrc/jpeg_decode.h). outRGBA8 == NULL asks for the
 * size. HPT_ERR_UNSUPPORTED for files outside that subset. Host code; no context. */
int  hpt_decode_jpeg(const uint8_t* file, uint64_t fileSize, uint32_t* outWidth, uint32_t* outHeight, uint8_t* outRGBA8, uint64_t outCapacity);
/* mi::fresnel_coat_precompute (mi_materials.cpp:377-451), what LoadPlasticMaterial (integrator_pt_scene_mat.cpp:675-757) stores for a
 * MAT_TYPE_PLASTIC: the 64-entry rough-transmittance table (appended to m_arrays1f, its offset in Material::datai[0]) and the two scalars
 * Material::data[PLASTIC_PRECOMP_REFLECTANCE = 3], data[PLASTIC_SPEC_SAMPLE_WEIGHT = 2]. Host code; no context, no device. RGB mode. */
int  hpt_plastic_precompute(float alpha, float intIor, float extIor, const float* diffuseReflectance4, const float* specularReflectance4,
                            float* outTransmittance64, float* outInternalReflectance, float* outSpecularSamplingWeight);
int  hpt_device_malloc(hpt_ctx* ctx, size_t bytes, void** outDev);
int  hpt_device_free(hpt_ctx* ctx, void* dev);
int  hpt_device_copy(hpt_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
int  hpt_device_memset(hpt_ctx* ctx, void* dev, int value, size_t bytes);

/* ---- ISceneObject: BVH2 replacement of the Embree backend (external/CrossRT/CrossRT.h:45-176) ------------------ */
int      hpt_clear_geom(hpt_ctx* ctx);                                                   /* ClearGeom            :56 */
uint32_t hpt_add_geom_triangles3f(hpt_ctx* ctx, const float* vpos3f, size_t vertNumber, const uint32_t* triIndices,
                                  size_t indNumber, uint32_t flags, size_t vByteStride); /* AddGeom_Triangles3f  :73-74; returns geomId or 0xFFFFFFFF */
int      hpt_update_geom_triangles3f(hpt_ctx* ctx, uint32_t geomId, const float* vpos3f, size_t vertNumber,
                                     const uint32_t* triIndices, size_t indNumber, uint32_t flags, size_t vByteStride); /* UpdateGeom_Triangles3f :85-86 */
int      hpt_clear_scene(hpt_ctx* ctx);                                                  /* ClearScene           :105 */
uint32_t hpt_add_instance(hpt_ctx* ctx, uint32_t geomId, const float matrix16[16]);      /* AddInstance          :118; returns instId or 0xFFFFFFFF */
/* AddInstanceMotion :127 (EmbreeRT.cpp:264-292): matrixNumber key transforms, linearly interpolated at the ray's time; 2 are supported
 * (what LoadSceneInstances passes). The automatic layout choice keeps two-level for scenes with a moving instance (the single-level layout
 * inverts the interpolated matrix per triangle record); both layouts and both schedules render them, bit-identically. */
uint32_t hpt_add_instance_motion(hpt_ctx* ctx, uint32_t geomId, const float* matrices /* matrixNumber x 16, column-major */, uint32_t matrixNumber);
int      hpt_update_instance(hpt_ctx* ctx, uint32_t instId, const float matrix16[16]);   /* UpdateInstance       :134 */
/* CommitScene :109-110. options = BuildOptions (CrossRT.h:8-14): BUILD_HIGH (4, the reference's default) or 0 build the tree with the host's binned-SAH
 * builder; BUILD_LOW (1) / BUILD_MEDIUM (2) without BUILD_HIGH build the single-level tree ON THE DEVICE (a linear BVH and its 4-wide compressed form,
 * milliseconds for 10^6 triangles: scenes whose topology changes every frame) when the scene takes the single-level layout (hpt_set_accel_layout) and no
 * instance moves; hpt_set_option("device_build", 1 / 0) forces / forbids that whatever the options say. Hits never depend on which builder ran. */
int      hpt_commit_scene(hpt_ctx* ctx, uint32_t options);
/* RayQuery_NearestHit / RayQuery_AnyHit (:148,:165), batched: n rays from host memory, results to host memory. */
int      hpt_ray_query_nearest(hpt_ctx* ctx, const float* posAndNear4, const float* dirAndFar4, uint32_t n, hpt_hit* out);
int      hpt_ray_query_any(hpt_ctx* ctx, const float* posAndNear4, const float* dirAndFar4, uint32_t n, uint32_t* out);
/* RayQuery_NearestHitMotion / RayQuery_AnyHitMotion (:157,:174): the same at a time in [0, 1] of the moving instances (one time per batch). */
int      hpt_ray_query_nearest_motion(hpt_ctx* ctx, const float* posAndNear4, const float* dirAndFar4, uint32_t n, float time, hpt_hit* out);
int      hpt_ray_query_any_motion(hpt_ctx* ctx, const float* posAndNear4, const float* dirAndFar4, uint32_t n, float time, uint32_t* out);

/* ---- scene tables --------------------------------------------------------------------------------------------- */
/* CommitDeviceData() (integrator_pt.h:265): uploads every scene vector. If desc->vPos4f is non-NULL the geometry
 * is (re)registered through the ISceneObject calls above in mesh / instance order and committed; otherwise the
 * acceleration structure committed earlier through hpt_add_geom_* / hpt_add_instance / hpt_commit_scene is used. */
int  hpt_upload_scene(hpt_ctx* ctx, const hpt_scene_desc* desc);
int  hpt_update_params(hpt_ctx* ctx, const hpt_params* params);                          /* UpdateMembersPlainData :268 */
int  hpt_update_materials(hpt_ctx* ctx, size_t first, size_t count, const void* mats);   /* Update_m_materials     :468 */
int  hpt_update_lights(hpt_ctx* ctx, size_t first, size_t count, const void* lights);    /* Update_m_lights        :469 */
/* Update_m_matIdOffsets() (integrator_pt.h:470): re-upload m_matVertOffset (uint2 x numGeoms: first triangle / first vertex of every mesh in
 * m_matIdByPrimId / m_triIndices and m_vData8f) after the host changed it; the ranges are checked against the uploaded tables. */
int  hpt_update_mat_id_offsets(hpt_ctx* ctx, const uint32_t* matVertOffset, size_t numGeoms);
int  hpt_pack_xy(hpt_ctx* ctx, uint32_t tidX, uint32_t tidY);                            /* PackXYBlock (integrator_pt_host.cpp:19-27) */
int  hpt_get_packed_xy(hpt_ctx* ctx, uint32_t* out, uint32_t count);
int  hpt_init_random_gens(hpt_ctx* ctx, uint32_t maxThreads);                            /* InitRandomGens (integrator_pt.cpp:13-21) */
/* The same seeding (RandomGenInit, crandom.h:25-36) for thread ids firstSeed .. firstSeed + maxThreads - 1: rank r of a sample-sharded
 * multi-GPU render seeds its generators as threads r * maxThreads ... of one big InitRandomGens call, i.e. decorrelated sub-streams. */
int  hpt_init_random_gens_from(hpt_ctx* ctx, uint32_t maxThreads, uint32_t firstSeed);
int  hpt_get_random_gens(hpt_ctx* ctx, uint32_t* outUint2, uint32_t count);              /* m_randomGens is integrator-owned, device copy authoritative */
int  hpt_set_random_gens(hpt_ctx* ctx, const uint32_t* inUint2, uint32_t count);

/* ---- the hot path --------------------------------------------------------------------------------------------- */
/* Integrator::PathTraceBlock(tid, channels, out_color, a_passNum) (integrator_pt.h:260, integrator_pt_host.cpp:57-73).
 * Processes tid in [tidBegin, tidBegin+tidCount) (the reference always passes the whole window: tidBegin = 0,
 * tidCount = W*H; a sub-range is what one rank of a multi-GPU job renders). out_color is the caller's full
 * W*H*channels host framebuffer; radiance is ACCUMULATED into it (+=), un-normalised, as in the reference. */
int  hpt_path_trace_block(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color, uint32_t passNum);
/* NaivePathTraceBlock (integrator_pt.h:259, integrator_pt_host.cpp:39-55) */
int  hpt_naive_path_trace_block(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color, uint32_t passNum);
/* Multi-GPU split of one frame (no reference counterpart: the reference is single-device). With stride > 1 the k-th work item of a
 * *_block call renders tid = tidBegin + (k / chunk) * chunk * stride + k % chunk, i.e. a rank passes tidBegin = rank * chunk and
 * renders every stride-th chunk of the tile-swizzled tid space (items past the viewport are dropped). chunk must be a multiple of 64
 * (one 8x8 tile). stride <= 1 restores the contiguous window [tidBegin, tidBegin + tidCount). */
int  hpt_set_tid_interleave(hpt_ctx* ctx, uint32_t chunk, uint32_t stride);
/* Same with the framebuffer already resident in device memory (kernel_slicer's generated class keeps out_color on the
 * device between calls, kmake_mega.json:18). stream is a hipStream_t (NULL = default stream); asynchronous. */
int  hpt_path_trace_block_dev(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color_dev,
                              uint32_t passNum, int naive, void* stream);
/* PathTraceFromInputRaysBlock(tid, channels, in_rayPosAndNear, in_rayDirAndFar, out_color, a_passNum) (integrator_pt.h:261,
 * integrator_pt.cpp:159-199, 761-798): the path tracer fed with the caller's rays (RayPosAndW / RayDirAndT, 16 bytes each, camera space:
 * cam_plugin/CamPluginAPI.h:27-37) instead of camera rays; out_color[tid * channels ..] += raw accumColor, m_randomGens[tid] advanced.
 * Needs hpt_init_random_gens(>= tid); no PackXYBlock. Host-pointer and device-pointer forms. */
int  hpt_path_trace_from_input_rays_block(hpt_ctx* ctx, uint32_t tid, uint32_t channels, const float* rayPosAndW, const float* rayDirAndT, float* out_color, uint32_t passNum);
int  hpt_path_trace_from_input_rays_block_dev(hpt_ctx* ctx, uint32_t tid, uint32_t channels, const float* rayPosAndWDev, const float* rayDirAndTDev, float* outDev, uint32_t passNum, void* stream);

/* ---- adaptive sampling (no counterpart in the reference) ---------------------------------------------------------------- */
/* One record per tid: the sums of the samples' luminance and of its square, in pass order, and the number of samples. The luminance of a sample
 * is y = (0.2126f * r + 0.7152f * g) + 0.0722f * b in f32 over the three values the sample adds to the frame (the one value when channels == 1).
 * Records accumulate across calls; a caller who wants fresh statistics zeroes the array. reserved is written as 0. */
typedef struct hpt_pixel_moments { float sumY; float sumY2; uint32_t passes; uint32_t reserved; } hpt_pixel_moments;
/* The planner's parameters. A pixel with n passes, mean m and variance v of its luminance asks for ceil(v / (tol * (|m| + lumFloor))^2) passes in
 * all, at least minPasses; a call gives it at most `step` more and never more than maxPasses in all. dilate = 1: a pixel asks for what the
 * neediest pixel of its 3 x 3 neighbourhood asks for (clipped to the frame; the neighbourhood stops at the edge of the tid window).
 * HPT_ERR_ARG unless tol and lumFloor are finite and > 0, 1 <= minPasses <= maxPasses, 1 <= step and dilate is 0 or 1. */
typedef struct hpt_adaptive_params { float tol; float lumFloor; uint32_t minPasses; uint32_t maxPasses; uint32_t step; uint32_t dilate; } hpt_adaptive_params;
/* What the planner and the loop report (32 bytes). The planner: passes = the sum of the counts it wrote, pixels = counts above 0, maxPasses = the
 * largest record's passes, nonfinite = records with passes whose sums are not finite (they are given no more), rounds = 0, deviceMs = 0.
 * The loop: passes = passes spent, pixels = pixels still short at the end, maxPasses and nonfinite of the final records, rounds = render
 * launches (the first included), deviceMs = the sum of their kernel times. */
typedef struct hpt_adaptive_info { uint64_t passes; uint32_t pixels; uint32_t maxPasses; uint32_t nonfinite; uint32_t rounds; float deviceMs; uint32_t reserved; } hpt_adaptive_info;
/* PathTraceBlock with a pass count per pixel. passCounts and moments are arrays of winWidth * winHeight entries indexed by absolute tid, like
 * m_randomGens; the window [tidBegin, tidBegin + tidCount) of them is read (and, of moments, written). passCounts NULL: passNum passes for every
 * pixel; otherwise passNum is not read. A pixel with count k ends, bit for bit, as a PathTraceBlock call with k passes leaves it (frame and
 * generator); a pixel with count 0 is neither read nor written. moments NULL: no statistics. Always the persistent megakernel with whole pixels:
 * hpt_set_schedule and the option "pass_slice" are ignored and hpt_get_last_launch reports schedule 1 (heavy scenes included).
 * HPT_ERR_UNSUPPORTED with a message, nothing touched: m_spectral_mode, scenes with thin films, naive != 0, the instrumented probe.
 * The device form is asynchronous on stream and honours hpt_set_tid_interleave (the arrays are indexed by the tids the items map to); the host
 * form copies the frame and the contiguous window of both arrays in, and the frame and moments out, and refuses a stride above 1 with
 * HPT_ERR_UNSUPPORTED. */
int  hpt_path_trace_block_counts(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color, uint32_t passNum,
                                 const uint32_t* passCounts, hpt_pixel_moments* moments);
int  hpt_path_trace_block_counts_dev(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color_dev, uint32_t passNum, int naive,
                                     const uint32_t* passCountsDev, hpt_pixel_moments* momentsDev, void* stream);
/* The planner: counts[tid] for the window from moments[tid] (both indexed by absolute tid), the totals in *info. Needs UpdateMembersPlainData and
 * PackXYBlock. The device form is asynchronous on stream; infoDev is device memory and is overwritten. */
int  hpt_adaptive_plan(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, const hpt_adaptive_params* params, const hpt_pixel_moments* moments,
                       uint32_t* passCounts, hpt_adaptive_info* info);
int  hpt_adaptive_plan_dev(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, const hpt_adaptive_params* params, const hpt_pixel_moments* momentsDev,
                           uint32_t* passCountsDev, hpt_adaptive_info* infoDev, void* stream);
/* out[pixel * channels + c] = frame[pixel * channels + c] / float(passes of the pixel's record) for c < min(channels, 3) over the window; a pixel
 * without passes is written as 0, a fourth channel is copied. Frames of winWidth * winHeight * channels floats (1, 3 or 4); out may be frame. */
int  hpt_adaptive_resolve(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, const float* frame, const hpt_pixel_moments* moments, float* out);
int  hpt_adaptive_resolve_dev(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, const float* frameDev, const hpt_pixel_moments* momentsDev,
                              float* outDev, void* stream);
/* The variance plane hpt_denoise_frame_var reads: outVar[y * winWidth + x] of every pixel of the window = the estimated variance of the pixel's
 * mean luminance, from its record {sumY, sumY2, n}: 0 without passes or with a sum that is not finite (such a pixel's colour is not finite
 * either and the filter rebuilds it); sumY * sumY for n = 1 (one sample shows no spread: 100 % relative error); otherwise
 * max(sumY2 / n - mean * mean, 0) / (n - 1) with mean = sumY / n, in f32 in this order. outVar: winWidth * winHeight floats; pixels outside the
 * window are not written. Needs PackXYBlock; HPT_ERR_ARG with a message for a null pointer or a window past the packed range, nothing written. */
int  hpt_adaptive_variance(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, const hpt_pixel_moments* moments, float* outVar);
int  hpt_adaptive_variance_dev(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, const hpt_pixel_moments* momentsDev, float* outVarDev, void* stream);
/* The loop, everything resident on the device: the window's records are zeroed, round 0 renders minPasses everywhere; then, up to maxRounds times:
 * plan, read the totals back, stop when nothing is asked for, render with the counts. out_color receives the un-normalised sums, as from
 * PathTraceBlock (hpt_adaptive_resolve divides them). moments may be NULL: the records then live in an array the context owns. Synchronous
 * (the totals are read between rounds); stream carries the launches. Refusals as hpt_path_trace_block_counts and the planner's, and
 * HPT_ERR_UNSUPPORTED under hpt_set_tid_interleave with a stride above 1 (the loop zeroes, plans and counts one contiguous window; a strided render
 * visits tids outside it). Every refusal is made before anything is written: frame, generators and the caller's records keep their contents. */
int  hpt_path_trace_block_adaptive(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color, const hpt_adaptive_params* params,
                                   uint32_t maxRounds, hpt_pixel_moments* moments, hpt_adaptive_info* info);
int  hpt_path_trace_block_adaptive_dev(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color_dev, const hpt_adaptive_params* params,
                                       uint32_t maxRounds, hpt_pixel_moments* momentsDev, hpt_adaptive_info* info, void* stream);

/* ---- G-buffer (integrator_gbuffer.cpp) ------------------------------------------------------------------------------- */
/* Integrator::GBufferPixel (integrator_pt.h:187-198): 15 dwords. A miss: depth 0, norm (0, 0, 1), ids -1, coverage 0. rgba[3] of a hit is
 * DEFINED as 1 (the reference reads color[3] of a float3 there, integrator_gbuffer.cpp:190: undefined); shadow is 0 (not implemented there). */
typedef struct hpt_gbuffer_pixel { float depth, norm[3], texc[2], rgba[4], shadow, coverage; int32_t matId, objId, instId; } hpt_gbuffer_pixel;
/* Integrator::EvalGBuffer(blockNum, out_gbuffer) (integrator_pt.h:251, integrator_gbuffer.cpp:243-267; main.cpp:269-277): for each of the
 * first blockNum pixels of m_packedXY, GBUFFER_SAMPLES = 16 pinhole primary rays at the pixel's Hammersley points (RayQuery_NearestHit, moving
 * instances at time 0), one record per ray, and GBufferReduction: the record most similar to the other fifteen, with the mean rgba of the
 * sixteen and its coverage estimate, written at out[y * winWidth + x]. out = winWidth * winHeight records in host memory; records of pixels
 * past blockNum are left as they are. Needs CommitDeviceData, CommitScene, UpdateMembersPlainData and PackXYBlock (else HPT_ERR_STATE); draws
 * no random numbers (no InitRandomGens), changes no state, works with m_spectral_mode on or off (it reads RGB base colours only). */
int  hpt_eval_gbuffer(hpt_ctx* ctx, uint32_t blockNum, hpt_gbuffer_pixel* out);
/* The same with the records resident in device memory; asynchronous on stream (a hipStream_t, NULL = default stream). samplesDev: NULL, or
 * 16 * blockNum records that receive every sample's record as it is before the reduction (sample k of packed pixel b at [16 * b + k]). */
int  hpt_eval_gbuffer_dev(hpt_ctx* ctx, uint32_t blockNum, hpt_gbuffer_pixel* outDev, hpt_gbuffer_pixel* samplesDev, void* stream);

/* DenoiseFrame: an edge-avoiding a-trous wavelet filter over a frame, guided by the records of EvalGBuffer. No counterpart in the reference
 * (it writes the records to images for an external denoiser); DESIGN.md 2.12 defines it operation by operation and
 * tests/denoise_reference.py restates it in numpy float32, bit for bit.
 *   iterations       1..8 passes of the 5 x 5 B3 kernel at tap distance 1, 2, 4, ... (default 5: a 125-pixel footprint)
 *   normalSquarings  0..8: the normal weight max(0, n_p . n_q) is squared this many times (default 7: power 128)
 *   flags            bit 0: divide the colour by max(albedo, 1e-3) before the filter and multiply it back after it (default on)
 *   normConst        scales the frame on the way in (1 / spp for an accumulated frame)
 *   sigmaColor, sigmaDepth, sigmaAlbedo   widths of the rational edge stops 1 / (1 + x); 0 switches a term off. Defaults 0.6, 0.05, 0.1:
 *                    chosen on the 4-spp Cornell box against its 512-spp frame (profiles/denoise.md).
 * A tap counts only where instId and matId equal the centre's; non-finite colours are skipped and rebuilt from their neighbours. */
typedef struct hpt_denoise_params { uint32_t iterations, normalSquarings, flags; float normConst, sigmaColor, sigmaDepth, sigmaAlbedo; } hpt_denoise_params;
#define HPT_DENOISE_DEMODULATE 1u
/* color4f: width * height pixels of 4 floats, row-major; gbuffer: width * height records in the same order (EvalGBuffer's for a full
 * window); out4f: width * height * 4 floats, rgb filtered, alpha = color alpha * normConst. Host pointers. Needs a created context only: no
 * scene, no PackXYBlock, no generators. HPT_ERR_ARG with a message naming the argument: a null pointer; width or height 0 (or above 32768);
 * iterations outside 1..8; normalSquarings above 8; a negative or non-finite sigma or normConst; unknown flag bits; out4f overlapping
 * color4f. hpt_get_execution_time("DenoiseFrame") gives its four slots. The scratch planes belong to the context and grow on demand. */
int  hpt_denoise_frame(hpt_ctx* ctx, uint32_t width, uint32_t height, const float* color4f, const hpt_gbuffer_pixel* gbuffer,
                       const hpt_denoise_params* params, float* out4f);
/* The same with the three arrays resident in device memory (params stays a host pointer); asynchronous on stream (a hipStream_t, NULL =
 * default stream): PathTraceBlock at low spp, EvalGBuffer and this call can follow each other on one stream. hpt_last_kernel_ms gives the
 * time of the pack kernel and the passes together. */
int  hpt_denoise_frame_dev(hpt_ctx* ctx, uint32_t width, uint32_t height, const float* color4fDev, const hpt_gbuffer_pixel* gbufferDev,
                           const hpt_denoise_params* params, float* out4fDev, void* stream);

/* DenoiseFrameVar: DenoiseFrame with the fixed colour stop replaced by a luminance stop scaled by each pixel's own estimated variance (SVGF,
 * Schied et al. 2017), fed by the records of adaptive sampling. DESIGN.md 2.12b defines it operation by operation and
 * tests/denoise_var_reference.py restates it in numpy float32, bit for bit. Everything of DenoiseFrame holds (taps, id and non-finite stops,
 * normal, depth and albedo terms, demodulation, alpha) except that params->sigmaColor must be 0; in its place
 *   x_l = (Y(c_p) - Y(c_q))^2 / (sigmaLum^2 * vbar_p + varFloor),  Y = (0.2126 r + 0.7152 g) + 0.0722 b,
 * where vbar_p is the pixel's variance (prefilter != 0: its 3 x 3 binomial mean at unit spacing). The variance plane is scaled like the colours
 * (normConst^2; under demodulation divided by the square of the floored albedo's luminance), travels through the passes as
 * sum(w^2 v_q) / (sum w)^2 and comes back in outVar.
 *   sigmaLum   width of the luminance stop in standard deviations; 0 switches the term off
 *   varFloor   added to the stop's denominator, above 0: what keeps it away from 0 where the variance is 0
 *   prefilter  0 or not 0;  reserved  0
 * The C interface has no defaults; the Python front end's were chosen on the 4-spp Cornell box (profiles/denoise_var.md). */
typedef struct hpt_denoise_var_params { float sigmaLum; float varFloor; uint32_t prefilter; uint32_t reserved; } hpt_denoise_var_params;
/* variance: width * height floats in pixel order (hpt_adaptive_variance's for a full window); an entry that is not finite or not above 0
 * counts as 0. outVar: NULL, or width * height floats that receive the filtered variance. The other arguments as hpt_denoise_frame. Host
 * pointers; needs a created context only. HPT_ERR_ARG with a message that names DenoiseFrameVar and the argument, nothing written: every refusal of
 * hpt_denoise_frame; a null variance or var_params; sigmaLum negative or not finite; varFloor not finite or not above 0; reserved not 0;
 * sigmaColor not 0; out4f overlapping color4f or variance; outVar overlapping color4f, gbuffer, variance or out4f.
 * hpt_get_execution_time("DenoiseFrameVar") gives its four slots. It shares DenoiseFrame's scratch planes and adds two of one float per pixel. */
int  hpt_denoise_frame_var(hpt_ctx* ctx, uint32_t width, uint32_t height, const float* color4f, const hpt_gbuffer_pixel* gbuffer, const float* variance,
                           const hpt_denoise_params* params, const hpt_denoise_var_params* var_params, float* out4f, float* outVar);
/* The same with the arrays resident in device memory (both parameter records stay host pointers); asynchronous on stream.
 * hpt_last_kernel_ms gives the time of the pack kernel and the passes together. */
int  hpt_denoise_frame_var_dev(hpt_ctx* ctx, uint32_t width, uint32_t height, const float* color4fDev, const hpt_gbuffer_pixel* gbufferDev, const float* varianceDev,
                               const hpt_denoise_params* params, const hpt_denoise_var_params* var_params, float* out4fDev, float* outVarDev, void* stream);

/* ---- primary-ray preview and Whitted ray tracing (integrator_rt.cpp) ------------------------------------------------- */
/* Integrator::CastSingleRayBlock(tid, out_color, a_passNum) (integrator_pt.h:254, integrator_pt_host.cpp:29-36, integrator_rt.cpp:33-53,
 * 116-161, 420-430; main.cpp:435-446; hydra_api/hydra_cpu.cpp:105): for each of the first tid pixels of m_packedXY one pinhole ray through
 * the pixel centre, RayQuery_NearestHit (moving instances at time 0) and colour = colors[GLTF_COLOR_BASE].w > 0 ? clamp(w, 0, 1) splat :
 * colors[GLTF_COLOR_BASE] * texture, ASSIGNED to out_color[(y * winWidth + x) * 4 + 0..2], the fourth float 0. out_color = winWidth *
 * winHeight * 4 floats in host memory; pixels past tid keep their contents. A miss assigns 0 to the four floats of its own pixel (the
 * reference writes out_color[tid] = 0 there, one float that races with the pixel owning it: DESIGN.md 7). a_passNum is unused, as in the
 * reference. Needs CommitDeviceData, CommitScene, UpdateMembersPlainData and PackXYBlock (else HPT_ERR_STATE naming the missing call); tid >
 * winWidth * winHeight and null pointers are HPT_ERR_ARG; tid = 0 does nothing. Draws no random numbers (no InitRandomGens), changes no
 * state, is the same with m_spectral_mode on or off. hpt_get_execution_time("CastSingleRayBlock") gives its four slots. */
int  hpt_cast_single_ray_block(hpt_ctx* ctx, uint32_t tid, float* out_color, uint32_t passNum);
/* Integrator::RayTraceBlock(tid, channels, out_color, a_passNum) (integrator_pt.h:263, integrator_pt_host.cpp:75-90, integrator_rt.cpp:55-82,
 * 164-299, 432-461; main.cpp:459-472): one deterministic Whitted path per pixel - up to m_traceDepth times kernel_RayTrace2 (at time 0)
 * and kernel_RayBounce: an emitter adds throughput * emission and ends the path; otherwise every entry of m_lights is lit as a point at
 * its pos behind a RayQuery_AnyHit shadow ray, and the path continues as a perfect mirror weighted alpha * colors[METAL] + (1 - alpha) *
 * colors[COAT]. No environment term, no random numbers. The result is ADDED to out_color[(y * winWidth + x) * channels + 0..2]. channels
 * 3 and 4 are served; 1 and 2 are HPT_ERR_ARG (the reference then writes over the neighbouring pixel and past the buffer: DESIGN.md 7);
 * above 4 nothing is written, as in the reference (HPT_OK). Other errors, a_passNum and the state it needs: as hpt_cast_single_ray_block.
 * hpt_get_execution_time("RayTraceBlock") gives raytraceTime's four slots. */
int  hpt_ray_trace_block(hpt_ctx* ctx, uint32_t tid, uint32_t channels, float* out_color, uint32_t passNum);
/* The same with the frame resident in device memory; asynchronous on stream (a hipStream_t, NULL = default stream). hpt_last_kernel_ms
 * gives the kernel time of the last call. */
int  hpt_cast_single_ray_block_dev(hpt_ctx* ctx, uint32_t tid, float* outDev, uint32_t passNum, void* stream);
int  hpt_ray_trace_block_dev(hpt_ctx* ctx, uint32_t tid, uint32_t channels, float* outDev, uint32_t passNum, void* stream);

/* ---- quasi-Monte-Carlo path tracing (mlt/integrator_qmc.{h,cpp}, mlt/rnd_qmc.{h,cpp}; `hydra --qmc`) ------------------ */
/* qmc::init: the 11 x 31 table of 31-bit Niederreiter base-2 generator-matrix columns, out[dim * 31 + bit]. qmc::rndFloat(pos, dim) is the
 * XOR of the columns the low 31 bits of pos select, plus one, times 2^-31 in float (it reaches 1.0). Host code; no context, no GPU. */
int  hpt_qmc_table(uint32_t out[341]);
/* IntegratorQMC::EnableQMC (integrator_qmc.cpp:11-86): out = { m_qmcDofDim, m_qmcSpdDim, m_qmcMotionDim, m_qmcMatDim, m_qmcLgtDim } for
 * a scene with (dof = lens radius > 0 or lens stack, spectral = m_spectral_mode, motion = moving instances); 0 = that draw stays with the
 * pseudo generator. Host code; no context, no GPU. */
int  hpt_qmc_layout(int dof, int spectral, int motion, uint32_t out[5]);
/* IntegratorQMC::PathTraceBlock(pixelsNum, channels, out_color, a_passNum) (integrator_qmc.cpp:284-315): S = min(2^32 - 1, pixelsNum *
 * a_passNum) samples of the Niederreiter sequence. Sample s takes its film position, lens point, time and the first bounce's material and
 * light numbers from the table (hpt_qmc_layout says which), everything else from generator s % N, N = the size InitRandomGens gave; its
 * pixel is x = min(uint(u0 * winWidth), winWidth - 1), y likewise from u1, and exposure * (colour * camRespoceRGB) is ADDED to that pixel
 * (channels 3 / 4: rgb; channels 1: the luma 0.2126 / 0.7152 / 0.0722). out_color = winWidth * winHeight * channels floats in host memory.
 * Samples s, s + N, s + 2N ... run in that order on generator s % N (what the reference computes on one thread: DESIGN.md 7); the sum
 * into a pixel is made with float atomics, so the frame is reproducible to rounding only. HPT_ERR_UNSUPPORTED for channels 2 and,
 * unless the option "qmc_spectral" is set (below), with m_spectral_mode on and for channels above 4; HPT_ERR_ARG for a null context or buffer and before InitRandomGens (N = 0); HPT_ERR_STATE before
 * CommitDeviceData, UpdateMembersPlainData or PackXYBlock. The megakernel schedule, unless the option "qmc_wavefront" (below) sends the call to the
 * wavefront schedule. hpt_get_execution_time("PathTraceBlockQMC") gives its four slots.
 * Spectral QMC (`hydra --qmc --spectral`) is opt-in: after hpt_set_option(ctx, "qmc_spectral", 1) a context with m_spectral_mode on is served
 * instead of refused (with m_spectral_mode off nothing changes). A sample then carries four wavelengths, SampleWavelengths of dimension
 * m_qmcSpdDim (hpt_qmc_layout; taken after the time sample), and SpectralCamRespoceToRGB(accumColor, wavelengths, rayFlags) takes the place of
 * the camRespoceRGB product: exposure * rgb is added for channels 3 / 4, its luma for channels 1. channels above 4 are wavelength layers of
 * winWidth * winHeight floats each: every one of the four wavelengths adds exposure * accumColor[i] to pixel y * winWidth + x of layer
 * min(int(channels * (lambda_i - LAMBDA_MIN) / (LAMBDA_MAX - LAMBDA_MIN)), channels - 1), with float atomics too. channels 2 stays
 * HPT_ERR_UNSUPPORTED; thin films whose tables are not of spectral size are HPT_ERR_ARG, as in PathTraceBlock. */
int  hpt_path_trace_qmc_block(hpt_ctx* ctx, uint32_t pixelsNum, uint32_t channels, float* out_color, uint32_t passNum);
/* The same on device memory, asynchronous on stream. sampleColorDev (4 floats per sample) and samplePixelDev (one uint32 per sample),
 * either both NULL or both S elements long, receive for sample index s the colour as it was added (rgb and 0; channels 1: the luma and three
 * zeros) and the pixel index y * winWidth + x: these records are bit-reproducible and let a caller compose a deterministic frame. outDev may
 * be NULL when the records are asked for; all three NULL is HPT_ERR_ARG. */
int  hpt_path_trace_qmc_block_dev(hpt_ctx* ctx, uint32_t pixelsNum, uint32_t channels, float* outDev, uint32_t passNum,
                                  float* sampleColorDev, uint32_t* samplePixelDev, void* stream);
/* The same with a third record: sampleWavesDev (4 floats per sample; NULL, or S elements long together with the other two records - alone it is
 * HPT_ERR_ARG) receives the sample's four wavelengths in spectral QMC (untouched in RGB). With channels above 4 the colour record is the four
 * exposure * accumColor[i], which the wavelengths place in their layers. hpt_path_trace_qmc_block_dev forwards here with NULL. */
int  hpt_path_trace_qmc_block_dev2(hpt_ctx* ctx, uint32_t pixelsNum, uint32_t channels, float* outDev, uint32_t passNum,
                                   float* sampleColorDev, uint32_t* samplePixelDev, float* sampleWavesDev, void* stream);
/* S of the two calls above for (pixelsNum, passNum): min(2^32 - 1, pixelsNum * passNum). Host code; no context. */
uint32_t hpt_qmc_sample_count(uint32_t pixelsNum, uint32_t passNum);

/* ---- Kelemen MLT in primary sample space (mlt/integrator_kmlt.cpp; `hydra`'s MLT mode) ---------------------------------- */
/* m_randsPerThread: floats of one primary-sample-space vector = AlignedSize(10 * traceDepth + 6, 16). Slots 0..3: the lens float4 (0 and 1
 * are the film position in [0,1]); 4: the wavelength sample (GetRandomNumbersSpec: SampleWavelengths of it gives a spectral path its four
 * wavelengths; not read in RGB); 5: the time; 6 + 10 b + 0..3: bounce b's light float4 (.w selects
 * the light); 6 + 10 b + 4..7: its material float4; 6 + 10 b + 8 + layer: its blend numbers (layer 2 and up overlaps the next bounce's light
 * numbers, as in the reference; a slot past the vector's end reads 0). Host code; no context, no GPU. */
uint32_t hpt_kmlt_state_size(uint32_t traceDepth);
/* IntegratorKMLT::PathTraceF for n vectors in device memory, vector i at xDev + i * strideFloats: the path whose every random number is read
 * from the vector. color4fDev[i] = accumColor * m_exposureMult and a fourth float 0 (no camRespoceRGB: PathTraceF applies none in RGB mode),
 * pixelDev[i] = y * winWidth + x with x = min(uint(x[0] * winWidth), winWidth - 1), y likewise from x[1] (IntegratorQMC::SampleCameraRay).
 * m_randomGens is neither read nor written. Asynchronous on stream. HPT_ERR_ARG for a null pointer or strideFloats below
 * hpt_kmlt_state_size(traceDepth); HPT_ERR_UNSUPPORTED with m_spectral_mode on unless the option "kmlt_spectral" is set (below);
 * HPT_ERR_STATE before CommitDeviceData, UpdateMembersPlainData or PackXYBlock. Megakernel schedule only.
 * Spectral MLT (`hydra --mlt --spectral`) is opt-in: after hpt_set_option(ctx, "kmlt_spectral", 1) (0 is the default, any other value
 * HPT_ERR_ARG) this entry, hpt_path_trace_kmlt_block and hpt_path_trace_kmlt_block_dev serve a context with m_spectral_mode on instead of
 * refusing it; with m_spectral_mode off nothing changes. A path then carries the four wavelengths SampleWavelengths(x[4]) and color4fDev[i] =
 * m_exposureMult * SpectralCamRespoceToRGB(accumColor, wavelengths, rayFlags): the chains' contribFunc, acceptance, contributions and
 * normalisation work on RGB as before. channels stays 4 (no wavelength layers); thin films whose tables are not of spectral size are
 * HPT_ERR_ARG, as in PathTraceBlock; the FB_DIRECT layer still forwards to the QMC entry, whose own option "qmc_spectral" decides there. */
int  hpt_path_trace_pss_dev(hpt_ctx* ctx, const float* xDev, uint32_t n, uint32_t strideFloats, float* color4fDev, uint32_t* pixelDev, void* stream);
/* The same with two more records of 4 floats per vector, each NULL or n elements long: waves4fDev[i] = the path's four wavelengths,
 * accum4fDev[i] = m_exposureMult * accumColor[k], the four raw components before SpectralCamRespoceToRGB. They exist in spectral MLT only: on
 * a context with m_spectral_mode off a non-NULL one is HPT_ERR_ARG. hpt_path_trace_pss_dev forwards here with NULLs. */
int  hpt_path_trace_pss_dev2(hpt_ctx* ctx, const float* xDev, uint32_t n, uint32_t strideFloats, float* color4fDev, uint32_t* pixelDev,
                             float* waves4fDev, float* accum4fDev, void* stream);
/* Records of the chains, all in device memory, each pointer NULL or long enough: per chain c and step i at [c * steps + i] - whether the step
 * was a large one and whether it was accepted (bytes), the acceptance probability a, the proposal's colour (4 floats) and pixel, the pixel of
 * the state it was compared with; per chain the initial state's colour and pixel; every proposal vector, [c][i][state size] floats; and
 * per chain and step the two contributions as formed, contribAtX (at the compared state) and contribAtY (at the proposal), 4 floats each, the
 * fourth 1 when the step added it to the frame (its squared length passed the 1e-12 test) and 0 when not.
 * C = the chain count, steps = (pixelsNum * passNum) / C. */
typedef struct hpt_kmlt_records {
  uint8_t*  isLarge;
  uint8_t*  accepted;
  float*    a;
  float*    color;
  uint32_t* pixel;
  uint32_t* oldPixel;
  float*    initColor;
  uint32_t* initPixel;
  float*    proposals;
  float*    contribAtX;
  float*    contribAtY;
} hpt_kmlt_records;
/* IntegratorKMLT::PathTraceBlock(pixelsNum, channels, out_color, a_passNum) (integrator_kmlt.cpp:248-478): C Markov chains of
 * (pixelsNum * a_passNum) / C steps each, every step adding its two contributions to the frame with float atomics, then the brightness
 * normalisation multiplies the first pixelsNum * 4 floats by normConst: pass a zero-filled frame of winWidth * winHeight * 4 floats. C is
 * hpt_set_option("kmlt_chains", n), by default one chain per lane of the resident grid, at most pixelsNum * a_passNum (DESIGN.md 7 has this
 * and the other definitions the reference ties to its thread count). m_randomGens is left untouched. m_renderLayer == FB_DIRECT forwards to
 * hpt_path_trace_qmc_block and returns what it returns. HPT_ERR_ARG for a null frame, channels other than 4, pixelsNum above winWidth *
 * winHeight and kmlt_chains above pixelsNum * a_passNum; HPT_ERR_UNSUPPORTED with m_spectral_mode on unless the option "kmlt_spectral" is
 * set (hpt_path_trace_pss_dev; the default chain count is then the spectral kernel's resident grid); HPT_ERR_STATE as hpt_path_trace_pss_dev;
 * a_passNum = 0 is HPT_OK and touches nothing. hpt_get_execution_time("PathTraceBlockKMLT") gives its four slots; the kernel slot spans the chains and the normalisation. */
/* C and steps = (pixelsNum * passNum) / C of a hpt_path_trace_kmlt_block call made now with these arguments (the option kmlt_chains, or the
 * resident grid of the present launch configuration, at most pixelsNum * passNum): what a caller sizes its record arrays by. Both 0 when
 * pixelsNum * passNum is 0; HPT_ERR_ARG where the call would refuse the chain count. Host code; no GPU work. */
int  hpt_kmlt_chain_count(hpt_ctx* ctx, uint32_t pixelsNum, uint32_t passNum, uint32_t* chains, uint32_t* steps);
int  hpt_path_trace_kmlt_block(hpt_ctx* ctx, uint32_t pixelsNum, uint32_t channels, float* out_color, uint32_t passNum);
/* The same on device memory, asynchronous on stream. normalize: 0 = the chains only (the frame holds the raw sums), 1 = the chains and the
 * normalisation, 2 = the normalisation alone, of the frame as it is and the chains of the last call on this context (so a caller can keep the
 * raw sums of the same run). recDev: host struct of device pointers, or NULL. stats4Dev, if not NULL, receives { avgBrightness (mean over the
 * chains that made a large step of their mean F over large steps), actualBrightness (mean contribFunc of the first pixelsNum pixels before
 * scaling), accepted steps / (pixelsNum * passNum), normConst }; normConst is 1 and nothing is scaled when no chain made a large step or the
 * frame is black. */
int  hpt_path_trace_kmlt_block_dev(hpt_ctx* ctx, uint32_t pixelsNum, uint32_t channels, float* outDev, uint32_t passNum,
                                   int normalize, hpt_kmlt_records* recDev, double* stats4Dev, void* stream);

/* ---- camera plug-in (cam_plugin/CamPluginAPI.h:39-77; CamPinHole.cpp, CamTableLens.cpp, main_with_cam_gpu.cpp) ----- */
/* The two ICamRaysAPI2 cameras of the reference on the device, and the loop that feeds PathTraceFromInputRaysBlock from them with rays, colours
 * and frame resident in device memory. A camera belongs to the context it was made from (its device, its error text: failures below are reported
 * through that context's hpt_last_error) and must be destroyed before it. Lane tid of a tile serves pixel p = subPassId * batchSize + tid
 * (x = p % width, y = p / width) and owns slot tid of the per-lane arrays m_randomGens, m_storedWaves, m_storedCos4, which chain from call to
 * call as in the reference. Everywhere: n <= batchSize and subPassId * batchSize + n <= width * height, else HPT_ERR_ARG (a short last tile
 * is allowed; the reference passes the batch size only); null pointers are HPT_ERR_ARG; rays or contributions before both
 * hpt_cam_set_parameters and hpt_cam_set_batch_size are HPT_ERR_ARG; a refused call leaves the camera as it was. */
typedef struct hpt_cam hpt_cam;
/* CamPinHole::CamPinHole / CamTableLens::CamTableLens: kind 0 = pinhole, 1 = table lens */
int  hpt_cam_create(hpt_ctx* ctx, int kind, hpt_cam** out);
void hpt_cam_destroy(hpt_cam* cam);
/* SetParameters(a_width, a_height, a_params) (CamPinHole.cpp:14-22, CamTableLens.cpp:60-68): projInv16 = inverse4x4(perspectiveMatrix(fov,
 * aspect, near, far)), column-major like hpt_params::projInv, made by the caller's matrix code; spectralMode = CamParameters::spectralMode. */
int  hpt_cam_set_parameters(hpt_cam* cam, uint32_t width, uint32_t height, const float* projInv16, int spectralMode);
/* `lines` and m_physSize of CamTableLens::Init (CamTableLens.cpp:87-112): lines4 = n x {curvatureRadius, thickness, eta, apertureRadius}, film
 * side first (the layout of hpt_set_optics; 1 .. 64 lines). A table-lens camera without lines makes no rays; a pinhole refuses the call. */
int  hpt_cam_set_lens(hpt_cam* cam, const float* lines4, uint32_t n, float physSizeX, float physSizeY);
/* SetBatchSize / Init(a_maxThreads) (CamPinHole.cpp:24-39, CamTableLens.cpp:70-85): allocates the per-lane arrays and the tile buffers on the
 * device; m_randomGens[i] = RandomGenInit(i + 12345 * i), the seed formed with 32-bit wrap-around and taken as int (the reference's int
 * overflows from i = 173 942: DESIGN.md 7); stored waves and cos4 start at 0. */
int  hpt_cam_set_batch_size(hpt_cam* cam, uint32_t tile);
/* MakeRaysBlock(out_rayPosAndNear4f, out_rayDirAndFar4f, in_blockSize, subPassId) (CamPinHole.cpp:41-96, CamTableLens.cpp:116-287): n camera-space
 * rays, RayPosAndW / RayDirAndT of 16 bytes each. Pinhole: through the pixel centre, origin 0; in spectral mode one rndFloat1 of slot tid gives
 * the wavelength. Table lens: one rndFloat4 of slot tid, a film point, a point on the rear element, the lens stack; a blocked ray is origin
 * (0, -1e7, 0), direction (0, -1, 0). Host-pointer form, and device-pointer form asynchronous on stream (a hipStream_t, NULL = default stream). */
int  hpt_cam_make_rays_block(hpt_cam* cam, float* rayPosAndW, float* rayDirAndT, uint32_t n, int subPassId);
int  hpt_cam_make_rays_block_dev(hpt_cam* cam, float* rayPosAndWDev, float* rayDirAndTDev, uint32_t n, int subPassId, void* stream);
/* AddSamplesContributionBlock(out_color4f, colors4f, in_blockSize, a_width, a_height, subPassId) (CamPinHole.cpp:46-50, 98-131,
 * CamTableLens.cpp:121-125, 289-319): out_color4f[p].rgb += colour of ray tid (times the stored cos^4 for the table lens), alpha untouched.
 * colors: 4 floats per ray; in spectral mode 1 float per ray, taken as four equal samples at the ray's stored wavelength through SpectrumToXYZ
 * (360, 830, the context's m_cie_xyz or, without a spectral scene, the loaders' table) and XYZToRGB; CamTableLens.cpp:309 calls a seven-argument
 * SpectrumToXYZ that does not exist: defined as the pinhole's call. width / height must be those of hpt_cam_set_parameters. */
int  hpt_cam_add_samples_contribution_block(hpt_cam* cam, float* out_color4f, const float* colors, uint32_t n, uint32_t width, uint32_t height, int subPassId);
int  hpt_cam_add_samples_contribution_block_dev(hpt_cam* cam, float* out_color4fDev, const float* colorsDev, uint32_t n, uint32_t width, uint32_t height,
                                                int subPassId, void* stream);
/* No counterpart in the reference: host copies of the first n slots of m_randomGens (uint32 pairs), m_storedWaves and m_storedCos4, for tests
 * and callers that checkpoint. Any of the three may be NULL. Synchronises the device. */
int  hpt_cam_read_state(hpt_cam* cam, uint32_t* gensUint2, float* waves, float* cos4, uint32_t n);
/* The loop of main_with_cam_gpu.cpp:230-266, `passes` times over the ceil(width * height / batchSize) tiles: zero the tile's colours,
 * MakeRaysBlock, PathTraceFromInputRaysBlock(n, channels, ..., a_passNum = 1), AddSamplesContributionBlock into frame4fDev (width * height * 4
 * floats, added to). channels = 1 in spectral mode, else 4. Everything is enqueued on `stream`; nothing waits for the device. Needs
 * hpt_init_random_gens(>= batchSize) and an integrator whose m_spectral_mode agrees with the camera's. */
int  hpt_cam_render_dev(hpt_ctx* ctx, hpt_cam* cam, float* frame4fDev, uint32_t passes, void* stream);
/* GetExecutionTime(a_funcName, a_out) (CamPluginAPI.h:76). "MakeRaysBlock" / "AddSamplesContributionBlock": the four slots of the last
 * host-pointer call, as hpt_get_execution_time; after hpt_cam_render_dev (which this call waits for) out[0] = that stage's kernel time summed
 * over the loop's first 256 tiles. "PathTraceFromInputRays": the same sum for the trace stage. "Render": out[0] = first to last event of the
 * whole loop, out[1] = tiles rendered, out[2] = tiles timed per stage. Unknown names leave out untouched. */
int  hpt_cam_get_execution_time(hpt_cam* cam, const char* funcName, float out[4]);

/* ---- differentiable rendering (diff_render/integrator_dr.h:42-47, 103) ------------------------------------------ */
int  hpt_put_diff_tex2d(hpt_ctx* ctx, uint32_t texId, uint32_t width, uint32_t height, uint32_t channels,
                        uint64_t* outOffset, uint64_t* outSize);                         /* PutDiffTex2D (integrator_dr.cpp:33-53) */
/* The environment map is registered like any texture: with hpt_set_option(ctx, "dr_environment", 1), hpt_put_diff_tex2d(ctx, m_envTexId, w, h, 4)
 * makes PathTraceDR / PathTraceVJP read the map from a_data - at the path's end and along the shadow ray of an env light sample whose texId
 * is the registered texture - and add d loss / d texel to a_dataGrad, taken per unit texel (exact at a black map; channel 3 is never read, its
 * gradient stays 0). w, h are the sizes the fetch uses. A one-channel registration of the environment map is HPT_ERR_ARG. */
int  hpt_reset_diff_tex(hpt_ctx* ctx);                                                   /* LoadSceneEnd (integrator_dr.cpp:24-31); also clears hpt_put_diff_lights */
/* Light-colour gradients (no counterpart in the reference). Registers lights [firstLight, firstLight + count) of the uploaded m_lights as
 * differentiable and appends 4 * count floats to the parameter vector, as hpt_put_diff_tex2d appends a texture: light firstLight + i owns
 * a_data[*outOffset + 4 i + 0..2], its RGB gain; float 4 i + 3 is padding (never read, its gradient stays 0). *outSize = 4 * count; the offset
 * must be a multiple of 4. PathTraceDR / PathTraceVJP (and their _dev forms) then evaluate such a light from intensity * gain - the frame and
 * m_randomGens are, bit for bit, those of a scene whose intensities were multiplied on the host - and add d loss / d gain to a_dataGrad, taken
 * per unit gain (exact at gain 0). Served by the megakernel and the wavefront schedule; an explicit block-local request is HPT_ERR_UNSUPPORTED.
 * HPT_ERR_ARG, nothing changed: count 0, a range past the uploaded lights, a second registration on the context, a misaligned offset, null
 * out-pointers. The registration survives hpt_update_lights; hpt_reset_diff_tex and a scene upload clear it. RayTraceDR ignores it. */
int  hpt_put_diff_lights(hpt_ctx* ctx, uint32_t firstLight, uint32_t count, uint64_t* outOffset, uint64_t* outSize);
/* IntegratorDR::PathTraceDR (integrator_dr.cpp:1135-1218). a_dataGrad is overwritten (zeroed first), out_color accumulated,
 * *outLoss receives the value the reference returns. Host-pointer form. */
int  hpt_path_trace_dr(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color, uint32_t passNum,
                       const float* refImg, const float* data, float* dataGrad, size_t gradSize, float* outLoss);
/* Device-pointer form: all four arrays resident; *lossAccumDev (one float, device) receives sum over samples of loss / passNum
 * (divide by W*H for the reference's return value); dataGradDev is ACCUMULATED into (zero it yourself). Asynchronous. */
int  hpt_path_trace_dr_dev(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color_dev, uint32_t passNum,
                           const float* refImgDev, const float* dataDev, float* dataGradDev, size_t gradSize, float* lossAccumDev, void* stream);
/* PathTraceVJP: the vector-Jacobian product of PathTraceDR's frame, for losses computed by the caller. No counterpart in the reference, whose
 * PathTraceDR differentiates the per-sample squared difference to a_refImg only. The call traces PathTraceDR's paths - the same random numbers,
 * records and colours, out_color accumulated and m_randomGens advanced bit for bit as by hpt_path_trace_dr - and seeds each sample's reverse
 * sweep with the caller's adjoint of the sample's pixel, a = adjImg[(y * winWidth + x) * channels + 0..2], rows in out_color's order (NOT
 * flipped as a_refImg is), instead of 2 (colour - ref):
 *   dataGrad[j] = sum over pixels, samples s and c = 0..2 of a_c * d C_s[c] / d data[j],  C_s the sample's colour as it is added to out_color.
 * Nothing is divided by passNum: it is the VJP of the frame as out_color receives it. An adjoint equal to 2 (colour - ref) gives PathTraceDR's
 * gradient term for term. No loss is computed. adjImg NULL: the frame is rendered through the DR kernels and nothing else happens - no sweep,
 * dataGrad (which may then be NULL) untouched. With hpt_set_option("dr_skip_nonfinite", 1) a sample whose colour is not finite adds neither
 * colour nor gradient. Host-pointer form: dataGrad (gradSize floats) is zeroed and overwritten, out_color accumulated into.
 * Refusals: PathTraceDR's, with its codes and messages (lens stack, motion, environment maps, non-lean materials, spectral mode, gradSize
 * smaller than what is registered); channels other than 3 or 4 (the stride of both out_color and adjImg), a NULL out_color or data, and an
 * adjImg with a NULL dataGrad or gradSize 0 are HPT_ERR_ARG. Runs under every schedule; hpt_get_execution_time("PathTraceVJP") gives its slots. */
int  hpt_path_trace_vjp(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color, uint32_t passNum,
                        const float* adjImg, const float* data, float* dataGrad, size_t gradSize);
/* Device-pointer form: dataGradDev is ACCUMULATED into with float atomics (zero it yourself). Asynchronous on stream. */
int  hpt_path_trace_vjp_dev(hpt_ctx* ctx, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out_color_dev, uint32_t passNum,
                            const float* adjImgDev, const float* dataDev, float* dataGradDev, size_t gradSize, void* stream);
/* IntegratorDR::RayTraceDR(tid, channels, out_color, a_passNum, a_refImg, a_data, a_dataGrad, a_gradSize) (integrator_dr.h:39-40,
 * integrator_dr.cpp:168-273, 372-459; drmain.cpp:204): the differentiable form of CastSingleRayBlock. Per pixel of the first tid entries of
 * m_packedXY: the pinhole ray through the pixel centre, RayQuery_NearestHit (moving instances at time 0), colour = colors[GLTF_COLOR_BASE].w > 0 ?
 * clamp(w, 0, 1) splat : colors[GLTF_COLOR_BASE] * texture - the texture fetched from a_data (Tex2DFetchAD) when it is registered with
 * PutDiffTex2D, a_data is not NULL and dr_grad_mode is 1, else with CastSingleRayBlock's sampler - and loss = dot3(colour - ref, colour - ref)
 * with ref = a_refImg[((winHeight - y - 1) * winWidth + x) * channels + 0..2]. A HIT assigns (colour, 0) to out_color[(y * winWidth + x) * 4 +
 * 0..3], at a stride of FOUR whatever channels is: out_color = winWidth * winHeight * 4 floats. A MISS leaves its pixel of out_color untouched;
 * its colour is 0 and its loss |ref|^2 (the reference returns before kernel_CalcRayColor: DESIGN.md 7). a_dataGrad (a_gradSize floats) is
 * zeroed and receives d loss / d a_data summed over the pixels (not divided by a_passNum, as in the reference); *outLoss = the per-pixel
 * losses, each divided by a_passNum, summed in float in tid order: the reference's return value, bit for bit. Host pointers.
 * channels other than 3 or 4 are HPT_ERR_ARG (three floats of a_refImg are read per pixel at that stride), as are tid > winWidth * winHeight, a
 * NULL out_color or a_refImg, a NULL a_dataGrad with a_gradSize > 0 and a_gradSize smaller than what is registered. tid = 0 zeroes the gradient
 * and returns loss 0. State it needs, spectral mode, random numbers: as hpt_cast_single_ray_block. hpt_get_execution_time("RayTraceDR") gives
 * its four slots. hpt_set_option("dr_grad_mode", 0) stands for the constructor's a_gradMode = 0: the pass renders and returns the loss through
 * the ordinary sampler and the gradient stays zero (integrator_dr.cpp:432-438); PathTraceDR does not read the option. */
int  hpt_ray_trace_dr(hpt_ctx* ctx, uint32_t tid, uint32_t channels, float* out_color, uint32_t passNum,
                      const float* refImg, const float* data, float* dataGrad, size_t gradSize, float* outLoss);
/* Device-pointer form, asynchronous on stream. dataGradDev is ACCUMULATED into with float atomics (zero it yourself; reproducible to rounding
 * only where two pixels share an element). lossPerPixelDev (NULL or tid floats) receives pixel i's loss at index i, bit-reproducible;
 * lossAccumDev (NULL or one float) is ADDED the sum of loss / passNum, reduced per wave and then by one float atomic per wave: reproducible to
 * rounding only. dataDev may be NULL (no texture is then fetched from it and no gradient written). */
int  hpt_ray_trace_dr_dev(hpt_ctx* ctx, uint32_t tid, uint32_t channels, float* outDev, uint32_t passNum, const float* refDev, const float* dataDev,
                          float* dataGradDev, size_t gradSize, float* lossPerPixelDev, float* lossAccumDev, void* stream);
/* AdamOptimizer<float>::step (diff_render/adam.h:43-62) on device arrays. */
int  hpt_adam_step_dev(hpt_ctx* ctx, float* stateDev, const float* gradDev, float* momentumDev, float* gSquareDev, size_t n, int iter, void* stream);
/* Image2D4fRegularizer(w, h, data, grad) (diff_render/integrator_dr.cpp:317-367; drmain.cpp:213-217): grad += d RegLossImage2D4f / d data,
 * the total-variation-like texture regulariser (rgb of a w x h x 4 texture), hand-derived instead of __enzyme_autodiff. Device pointers. */
int  hpt_image2d4f_regularizer_dev(hpt_ctx* ctx, int w, int h, const float* data, float* grad, void* stream);
int  hpt_image2d4f_regularizer(hpt_ctx* ctx, int w, int h, const float* data, float* grad);       /* host pointers, the reference's signature */

/* ---- timing / instrumentation ----------------------------------------------------------------------------------- */
/* GetExecutionTime(name, out[4]) (integrator_pt.h:266, main.cpp:416-419): out[0] exec ms, [1] host->device, [2] device->host, [3] overhead */
int  hpt_get_execution_time(hpt_ctx* ctx, const char* funcName, float out[4]);
/* Counters of the last hpt_*_block call made with instrumentation enabled: [0..7] = {rays, nodesVisited, trisTested,
 * surfaceHits, shadowRays, paths, instancesEntered, texFetches} (feeds the algorithmic-bytes roofline);
 * [8..12] = wave-cycles (s_memtime) spent in {queue+regeneration, closest-hit traversal, shading, shadow traversal, path end},
 * [13] = bounce-loop trips summed over waves, [14] / [15] = wave-level iterations of the inner-node / triangle loops
 * (lane utilisation of traversal = [1] / (64 * [14]), [2] / (64 * [15])). The instrumented kernel is a separate build: never timed. */
int  hpt_set_instrumentation(hpt_ctx* ctx, int enabled);
int  hpt_get_counters(hpt_ctx* ctx, uint64_t out[16]);
/* The instrumented PathTraceDR launch (hpt_set_instrumentation(1) before hpt_path_trace_dr*; megakernel schedule) also fills: out[0] = adjoint
 * records stored (one per bounce), out[1] = of those with a parameter texture (gradient taps), out[2] / out[3] = wave-cycles of the record
 * stores / of the reverse sweeps (same clock as hpt_get_counters' phase slots, whose "path end" slot then excludes them), out[4] = wave-trips
 * that ran a sweep, out[5] = lanes in those sweeps, out[6] = atomic wave-instructions issued, out[7] = bounces the sweeps walked,
 * out[8] = records written to HBM (a path's last record stays in registers when the path ends in the same trip); out[9..15] reserved (0).
 * No counterpart in the reference (diff_render/integrator_dr.cpp:1135-1218 has no profile hooks). */
int  hpt_get_dr_counters(hpt_ctx* ctx, uint64_t out[16]);
/* Launch geometry of the persistent kernel: blocks per CU (0 = automatic). */
int  hpt_set_launch_config(hpt_ctx* ctx, int blocksPerCU);
/* Acceleration-structure layout chosen at the next hpt_commit_scene: 0 = automatic (the triangle sweep for scenes of <= 32 instanced
 * triangles, one world-space BVH2 over all instanced triangles for heavy static scenes, scenes from 4 096 instanced triangles and scenes of
 * six or more instances, else two-level), 1 = force the two-level TLAS/BLAS layout, 2 = force the single-level one, 3 = force the sweep
 * (no tree: every wave tests every triangle, fetched with scalar loads; cost linear in the triangle count).
 * All layouts intersect triangles in object space with the same arithmetic and return bit-identical hits. */
int  hpt_set_accel_layout(hpt_ctx* ctx, int layout);
/* How hpt_path_trace_block(_dev) schedules the work: 1 = one persistent megakernel (a lane keeps its path from camera to end),
 * 2 = wavefront (a shade kernel and a persistent trace kernel with ballot/prefix-sum ray compaction and ray replacement, path state
 * in HBM), 3 = the megakernel with block-local ray repacking (the rays of a workgroup's 256 lanes pooled in LDS and drained by its four
 * waves with replacement; gltf / emissive scenes, PathTraceDR and spectral rendering), 4 = the wavefront schedule in one launch (every workgroup
 * owns a tile-interleaved set of pool slots for the whole call and alternates between shading them and draining its own ray queue; heavy static gltf /
 * emissive scenes on the 4-wide tree - elsewhere the automatic choice is taken; never chosen automatically), 0 = automatic: wavefront when the committed BVH is
 * expected to cost a ray >= 20 inner-node visits (hpt_get_accel_info's surface-area estimate) and the call has >= 2^19 pixels, the
 * block-local form for lean scenes from an estimate of 8, else the plain megakernel. All give bit-identical frames. refillBelow (1..64,
 * 0 = keep): a trace wave refills from the ray queue when fewer lanes than this still hold a ray; traceBlocksPerCU 0 = automatic.
 * groups (0 = automatic): the pixels of a call are cut into this many groups with their own path pool, ray queue and HIP stream, so
 * that the tail of one group's trace pass (a few long rays) overlaps the other groups' shade and trace passes.
 * The naive integrator and input-ray batches always use the megakernel (scenes with moving instances run under either); PathTraceDR follows the same
 * automatic choice as PathTraceBlock (its wavefront form keeps the adjoint records per pool slot), and so does spectral rendering (m_spectral_mode = 1:
 * its own shade kernel with four samples per radiance word in front of the same trace kernel). The wavefront call returns once the frame is nearly done
 * (it polls a device progress word); results are complete after the stream is synchronised, as for the megakernel. */
int  hpt_set_schedule(hpt_ctx* ctx, int schedule, int refillBelow, int traceBlocksPerCU, int groups);
/* Tuning knobs without a place in the reference's interface (results never depend on them):
 *   "wf_grace"  trips a wavefront trace wave keeps going after the ray queue ran dry before it parks its unfinished rays (traversal
 *               state + stack to HBM) for the next round's trace pass, which resumes them first; 0 = run every ray to the end.
 *               Only applied in rounds with at least 2 rays per lane of the trace grid.
 *   "refit"     1 (default): CommitScene after UpdateInstance / UpdateGeom_Triangles3f refits the single-level tree on the device; 0: rebuild.
 *   "device_refit"  0 (default): an update of a DEVICE-built single-level tree is answered by another device build; 1: the device build leaves
 *               its level lists behind and such an update refits the tree (instance matrices and vertex positions; "refit", 0 still rebuilds).
 *               Read when the tree is built and again when the update is committed.
 *   "device_build_quality"  p: 0 (default) = a device build leaves the plain linear BVH; 1 .. 4 = it runs p passes of treelet restructuring over the
 *               hierarchy before the tree is emitted (every inner node with up to 7 descendants as leaves: the optimal topology over them by the
 *               surface-area cost, rewritten when strictly cheaper). Applies to every device build - "device_build" 1, BUILD_LOW | BUILD_MEDIUM, the
 *               build after a rejected refit, the rebuild of a device-built tree - and never to the host's. Anything else is an argument error.
 *               Setting it uncommits the scene, as "device_build" does. Hits do not depend on it; hpt_get_build_info says what the passes did.
 *   "device_build_two_level"  0 (default): scenes that take the two-level layout (a moving instance, hpt_set_accel_layout(ctx, 1), more instanced
 *               triangles than the single-level budget) are built by the host whatever is asked; 1: when a device build is asked for ("device_build" 1,
 *               or BUILD_LOW | BUILD_MEDIUM without BUILD_HIGH) and the scene is no triangle sweep and has a triangle, the BLAS of all meshes are
 *               built by ONE batched linear-BVH build in object space and the TLAS over the live instances by a second one. A later commit that
 *               only saw hpt_update_instance rebuilds the TLAS alone (BLAS nodes and all triangle records stay byte for byte); one that saw
 *               hpt_update_geom_triangles3f with unchanged indices rebuilds those meshes' BLAS in their slots, then the TLAS; anything else is a
 *               full device build ("refit", 0 forces that too). A tree deeper than the traversal stack goes to the host's builder as a whole.
 *               No treelet passes, no 4-wide form, no shading records on this layout. Anything but 0 / 1 is an argument error; setting it
 *               uncommits the scene. Hits do not depend on it; hpt_get_two_level_info says what the last commit did.
 *   "refit_max_sah_pct"  p: 0 (default) = never; p >= 100: a refit whose surface-area estimate (hpt_get_refit_info) exceeds p / 100 times the
 *               estimate at build time is followed, in the same hpt_commit_scene, by a build (on the device for a device-built tree, on the host
 *               for a host-built one). 1 .. 99 is an argument error.
 *   "node_min"  voted exit of the inner-node loop (0..63, applied at the next hpt_commit_scene; default chosen per scene).
 *   "pass_slice"  PathTraceBlock under the persistent megakernel (not NaivePathTrace, not scenes with thin films): n > 0 hands a pixel out in work items of n passes; the pixel's
 *               value and generator pass from item to item through device memory in pass order, so the frame and m_randomGens are bit for bit
 *               those of n = 0 (a work item is a whole pixel). n >= a_passNum is n = 0. PathTraceDR, PathTraceFromInputRays and the other
 *               schedules ignore it. A waiting lane that exceeds its poll limit makes the call (or, for the device-pointer forms, the next
 *               call or hpt_last_kernel_ms) return HPT_ERR_STATE. The limit counts polls (about 3 us each when a whole wave waits; at least 2^20),
 *               not time: with n set by hand on a heavy scene a healthy call could reach it. Never set: in calls with at least two and fewer than eight pixels per lane of the
 *               grid and at least 256 passes, 128 when that leaves a lane 32 work items or more and 64 when not; else 0. Environment: HPT_PASS_SLICE.
 * A member of the reference that is set in its constructor:
 *   "dr_grad_mode"  IntegratorDR's a_gradMode (integrator_dr.h; default 1). 0: RayTraceDR renders and returns the loss through the ordinary
 *               sampler and writes no gradient (integrator_dr.cpp:99, 432-438). PathTraceDR does not read it.
 *   "dr_environment"  0 (default): PathTraceDR / PathTraceVJP refuse a scene with an environment map, its sampling or a camera back plate
 *               (HPT_ERR_UNSUPPORTED). 1: scenes with m_envTexId and / or m_envEnableSam are served, as the reference's replay renders them
 *               (diff_render/integrator_dr.cpp:744-787, 1077-1098): every path end adds m_envColor * map along its final direction - times the
 *               env-sampling MIS weight under MIS with m_envEnableSam after a non-specular vertex (not on a primary miss), 0 under the shadow
 *               integrator with m_envEnableSam - and the LIGHT_GEOM_ENV light is sampled at every bounce. A registered map's texel gradient
 *               comes back in a_dataGrad (hpt_put_diff_tex2d). Still HPT_ERR_UNSUPPORTED: a camera back plate (the replay has none),
 *               hpt_put_diff_lights on the same context, an explicit block-local schedule (the automatic choice avoids it), the instrumented
 *               probe, spectral, lens and motion scenes. Scenes without a map run the kernels they always ran. Any other value: HPT_ERR_ARG.
 * Which schedule serves QMC path tracing (sample records and m_randomGens never depend on it; the frame is an atomic sum under either):
 *   "qmc_wavefront"  0 (default): hpt_path_trace_qmc_block[_dev, _dev2] - and the FB_DIRECT forward of hpt_path_trace_kmlt_block[_dev] - run the
 *               megakernel whatever hpt_set_schedule says. 1: such a call goes to the wavefront schedule exactly when a PathTraceBlock of as many
 *               pixels as it has generator slots with work, min(N, S) with S = hpt_qmc_sample_count(pixelsNum, passNum), would - schedule 0: the
 *               automatic rule, 2: always, 1 and 3: never, 4: the automatic rule. A pool slot is a generator slot and runs its samples g, g + N,
 *               ... in order, so every sample record and every generator is the megakernel's bit for bit. Kept on the megakernel, silently and
 *               with the same results: m_spectral_mode ("qmc_spectral" included), the triangle-sweep layout, RGB scenes with thin films, trace
 *               depth 0 and instrumented contexts. hpt_get_last_launch and hpt_get_schedule report what ran. A call that would take the wavefront
 *               form and whose slot 0 has more than 16777215 (0xFFFFFF) samples - what a pool slot's status word holds - returns HPT_ERR_ARG
 *               and writes nothing. What the entry refuses it refuses under either value. Any other value: HPT_ERR_ARG.
 * Which schedule serves adaptive sampling (results never depend on it):
 *   "adaptive_wavefront"  0 (default): hpt_path_trace_block_counts[_dev] and every round of hpt_path_trace_block_adaptive[_dev] run the megakernel
 *               whatever hpt_set_schedule says. 1: each such call goes to the wavefront schedule exactly when a PathTraceBlock of as many pixels
 *               as the call has pass counts above 0 would - schedule 0: the automatic rule, 2: always, 1 and 3: never, 4: the automatic rule - and
 *               hpt_get_last_launch reports what ran. Frame, m_randomGens and moments are bit for bit the megakernel's. The bare counts entry
 *               counts its array on the device first (12 bytes read back before anything is written); the loop decides per round from its
 *               own plan. A pool slot holds 24 bits of passes: a call that would run the wavefront form with a count above 16777215 (0xFFFFFF),
 *               and a loop whose minPasses or min(step, maxPasses) exceeds it, return HPT_ERR_ARG and write nothing. Counts that are all 0
 *               return HPT_OK and write nothing. What adaptive sampling refuses (spectral mode without "adaptive_spectral", thin films in RGB
 *               scenes, the naive integrator, input rays, the instrumented probe) it refuses under either value. Any other value: HPT_ERR_ARG.
 * Adaptive sampling under m_spectral_mode (off by default, as "qmc_spectral" and "kmlt_spectral" are):
 *   "adaptive_spectral"  0 (default): hpt_path_trace_block_counts[_dev] and hpt_path_trace_block_adaptive[_dev] refuse a context in spectral mode
 *               (HPT_ERR_UNSUPPORTED, nothing written). 1: they are served there, thin-film, dispersive and moving-instance scenes included: a pixel
 *               given k passes ends, frame and m_randomGens, bit for bit as a uniform spectral hpt_path_trace_block of k passes leaves it, a
 *               pixel with count 0 keeps every bit, and a record receives per sample the Rec. 709 luminance of the three values added to the
 *               frame (exposure * rgb after the camera response; the one value added with channels == 1), f32 in pass order.
 *               hpt_adaptive_plan / _resolve / _variance and hpt_denoise_frame_var read such records as they read RGB ones. The calls run the
 *               one-thread-per-pixel spectral kernel whatever hpt_set_schedule says (hpt_get_last_launch: schedule 1); with "adaptive_wavefront" 1
 *               as well they take the wavefront schedule under the rule stated there, where the spectral wavefront kernels apply (no moving
 *               instances, no sweep layout, trace depth above 0), with the same 24-bit limit and the same bits. Still HPT_ERR_UNSUPPORTED with
 *               nothing written: the naive integrator, input rays, the instrumented probe, channels > 4 (a moment over wavelength layers
 *               has no definition) and thin films in an RGB scene. Any other value: HPT_ERR_ARG.
 * Diagnostic switches (these DO change which kernels run or what they compute; never set in production):
 *   "dr_skip_nonfinite"     PathTraceDR: 1 = a sample whose radiance is not finite contributes neither colour, loss nor gradient (what an
 *                           optimisation loop wants: one NaN poisons Adam's moments for good); 0 (default) = PixelLossPT as the reference
 *                           has it, which adds every sample (diff_render/integrator_dr.cpp:1124-1131)
 *   "shade_records"         0: gltf / emissive scenes on the single-level layout gather vertex data through the index chain instead of the 64-byte
 *                           per-triangle shading records (kernel studies; environment: HPT_SHADE_RECORDS=0)
 *   "build_threads"         n: host threads CommitScene builds its trees with (meshes in parallel, big trees split into subtrees); 0 = the cores this
 *                           process may use, at most 16. The tree is the same whatever n is (only the numbering of its nodes differs)
 *   "wide_nodes"            0: the wavefront trace kernel walks the BVH2 instead of the 4-wide compressed tree of static single-level scenes
 *                           (kernel studies; environment: HPT_WIDE_NODES=0)
 *   "stats_wide"            1: the instrumented probe (hpt_set_instrumentation) counts the walk over the 4-wide tree
 *   "force_full_materials"  1: never pick the kernels specialised for gltf + emissive scenes (kernel studies)
 *   "dbg_no_normal_lerp"    1: moving instances without the reference's normal interpolation (integrator_pt.cpp:285-292); the checker has the
 *                           same switch (ORC_DBG_NO_NORMAL_LERP) - used to show where the rare path divergences under motion blur come from
 *   "dbg_stack_witness"     1: before every launch that walks a tree (path tracing under any schedule, ray queries, the G-buffer, primary-ray,
 *                           Whitted, RayTraceDR, QMC, primary-sample-space and KMLT passes) the HBM part of the traversal stacks is filled, on the
 *                           launch's stream, with a word no traversal pushes; hpt_get_stack_witness then counts the words the launch wrote. The
 *                           kernels and their results are the same; 0 (default): no fill, nothing else either. For tests of the deep stacks */
int  hpt_set_option(hpt_ctx* ctx, const char* name, int value);
/* ---- multi-GPU: one context = one GPU = one rank -----------------------------------------------------
 * The path shards without a data-path exchange; these three calls are the only traffic over xGMI. RCCL is loaded on first use.
 *   hpt_comm_get_unique_id : ncclGetUniqueId (128 bytes) on rank 0; the host distributes it (MPI, sockets, a file ...)
 *   hpt_comm_init          : ncclCommInitRank for this context's device
 *   hpt_reduce_framebuffer : in-place ncclReduce(sum, fp32) of the zero-initialised framebuffers to `root`, once per frame
 *   hpt_allreduce_grad     : in-place ncclAllReduce(sum, fp32) of a_dataGrad (or the one-float loss), once per optimisation iteration */
int  hpt_comm_get_unique_id(hpt_ctx* ctx, void* id128);
int  hpt_comm_init(hpt_ctx* ctx, int nranks, int rank, const void* id128);
int  hpt_comm_destroy(hpt_ctx* ctx);
int  hpt_reduce_framebuffer(hpt_ctx* ctx, float* frameDev, size_t count, int root, void* stream);
int  hpt_allreduce_grad(hpt_ctx* ctx, float* gradDev, size_t count, void* stream);
/* What CommitScene built: out[0] = expected inner-node visits per ray (surface-area estimate over the committed BVH; the quantity the automatic
 * schedule / layout choice is measured against), out[1] = instanced triangles, out[2] = instances, out[3] = layout (0 two-level, 1 single-level, 2 triangle sweep). */
int  hpt_get_accel_info(hpt_ctx* ctx, float out[4]);
/* The last hpt_commit_scene: out[0] = host milliseconds (BVH build, or for a refit the matrix inversions and record updates), out[1] = upload ms,
 * out[2] = device refit ms, out[3] = 1 when the committed single-level tree was REFITTED on the device (UpdateInstance / UpdateGeom_Triangles3f
 * with unchanged topology: triangle boxes, then one small kernel per tree level from the leaves up, then the 4-wide nodes requantised and the
 * tree's cost summed, CrossRT.h:85-86, 134; a host-built tree always, a device-built one under hpt_set_option("device_refit", 1)), 2 when it was
 * BUILT on the device (out[2] = the build's milliseconds) and 0 when it was built on the host. hpt_set_option("refit", 0) forces the build. */
int  hpt_get_commit_time(hpt_ctx* ctx, float out[4]);
/* The committed single-level tree's surface-area estimate before and after refits (a refit keeps the topology, so the tree degrades as objects
 * move; this is the number from which to decide on a rebuild): out[0] = the estimate at build time (hpt_get_accel_info's out[0]), out[1] = the
 * estimate of the tree as the last refit left it, summed on the device over the refitted boxes (= out[0] when the last commit was a build),
 * out[2] = number of levels a refit launches (0: the tree cannot be refitted), out[3] = 1 when the last hpt_commit_scene attempted a refit and
 * "refit_max_sah_pct" rejected it. Schedule and kernel choices keep following out[0]. */
int  hpt_get_refit_info(hpt_ctx* ctx, float out[4]);
/* The treelet passes of the last hpt_commit_scene when it was a device build (hpt_set_option("device_build_quality", p)): out[0] = passes run
 * (fewer than p when the tree has a single node, or is deeper than the level lists reach and goes back to the host's builder), out[1] = treelets of
 * three leaves or more examined over all passes, out[2] = treelets rewritten, out[3] = device milliseconds spent in the passes (contained in
 * hpt_get_commit_time's out[2]). All zeros after a host build, a refit, or with the option at 0. */
int  hpt_get_build_info(hpt_ctx* ctx, float out[4]);
/* Host copy of the committed single-level tree as it lies in device memory (tests, checkpoints; the counterpart of hpt_cam_read_state):
 * what = 0: the BvhNode array (64-byte records: q[12] = child 0 {lo.x hi.x lo.y hi.y lo.z hi.z}, child 1 {same}; ref0, ref1, two pad words),
 * what = 1: the BvhTri array (48-byte records: v0[3], primId, e1[3], instId, e2[3], pad). A reference with bit 31 set is a leaf
 * (bits 28..30 = triangle count, bits 0..27 = first record), 0xFFFFFFFE is "no child", anything else indexes the node array; *outRootRef
 * receives the root's reference. A device-built tree's node array has unused entries (only what the root reaches is a node).
 * dst == NULL: only *outBytes is set. HPT_ERR_ARG when capacityBytes is too small, HPT_ERR_STATE when no single-level tree is committed
 * (the two-level and sweep layouts are not read back). */
int  hpt_read_accel(hpt_ctx* ctx, int what, void* dst, uint64_t capacityBytes, uint64_t* outBytes, uint32_t* outRootRef);
/* The last hpt_commit_scene when it built the two-level layout on the device (hpt_set_option("device_build_two_level", 1)): out[0] = 1,
 * out[1] = BLAS built by that commit, out[2] = BLAS kept from earlier commits, out[3] = 1 when it rebuilt only the TLAS, out[4] = inner levels
 * of the TLAS, out[5] = of the deepest BLAS, out[6] / out[7] = device milliseconds of the BLAS / TLAS stage (between device events; contained in
 * hpt_get_commit_time's out[2]). All zeros after any other kind of commit. */
int  hpt_get_two_level_info(hpt_ctx* ctx, float out[8]);
/* Host copy of the committed two-level tree (either builder's) as it lies in device memory, with hpt_read_accel's conventions: what = 0 the BvhNode
 * array (the TLAS first; an instance leaf is a reference with bit 31 set, count bits 0 and the instance id in bits 0..27), what = 1 the BvhTri
 * array (every mesh's records in its BLAS' leaf order, instId 0), what = 2 the BvhInst array (64-byte records: three world -> object rows of four
 * floats, the mesh's BLAS root as a reference into the two arrays, geomId, 1 for a moving instance, a pad word). *outRootRef receives the TLAS
 * root. A device-built tree's node array has unused entries (the TLAS region past its nodes, slots of subtrees folded into leaves): zeros after a
 * full build, stale nodes after an in-place update; only what the roots reach is a node. HPT_ERR_STATE unless a two-level tree is committed. */
int  hpt_read_accel_two_level(hpt_ctx* ctx, int what, void* dst, uint64_t capacityBytes, uint64_t* outBytes, uint32_t* outRootRef);
/* Schedule the last hpt_path_trace_block(_dev) call used (1 .. 4, as hpt_set_schedule numbers them) and, for the wavefront one, its number of
 * shade+trace rounds. */
int  hpt_get_schedule(hpt_ctx* ctx, int* lastSchedule, uint32_t* lastIterations);
/* What the last hpt_path_trace_* call walked (no counterpart in the reference: lets a test assert WHICH kernels produced a frame):
 * out[0] = schedule (1 .. 4), out[1] = 1 when rays walked the 4-wide compressed tree, out[2] = 1 when surface data came from the 64-byte
 * shading records, out[3] = 1 when the traversal stacks had an HBM part, out[4] = passes per work item ("pass_slice"; 0 = whole pixels). */
int  hpt_get_last_launch(hpt_ctx* ctx, uint32_t out[5]);
/* With hpt_set_option("dbg_stack_witness", 1): out[0] = words of the traversal stacks' HBM part that no longer hold the fill word after the last
 * launch, i.e. that a lane pushed (the stack entries beyond the ones kept in LDS), out[1] = words that were filled before it. Waits for the device,
 * copies the buffer and counts on the host; it does not interpret the buffer's layout (the wavefront schedule's per-group slices count alike).
 * Without the option both are 0. 'Last launch' is literal: a launch that walks no tree refills the buffer too (hpt_path_trace_kmlt_block_dev with
 * normalize = 2, the normalisation alone), and after it out[0] is 0. */
int  hpt_get_stack_witness(hpt_ctx* ctx, uint64_t out[2]);
/* Duration of the last path-tracing or G-buffer kernel, measured with HIP events on the stream it ran on (ms). */
int  hpt_last_kernel_ms(hpt_ctx* ctx, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* HYDRA_HIP_H */
