// vqhip_passes.hpp — host-side C++ mirror of the reference's render-pass interface for the hot path.
//
// VQEngine's passes derive IRenderPass / RenderPassBase (Source/Renderer/Rendering/RenderPass/RenderPass.h:44-89) and take
// nested POD `FResourceCollection` / `FDrawParameters` structs (idiom: ApplyReflections.h:29-39, static_cast in
// RecordCommands: ApplyReflections.cpp:45-50). The four functions on the hot path are NOT behind that interface in the
// reference — they are VQRenderer members:
//     RenderSceneColor          Source/Renderer/Rendering/SceneRendering.cpp:1619
//     RenderPostProcess         SceneRendering.cpp:2507
//     PreFilterEnvironmentMap   Source/Renderer/Rendering/EnvironmentMapRendering.cpp:139
//     ComputeBRDFIntegrationLUT Source/Renderer/Renderer.cpp:871
// These adaptors give them the IRenderPass shape so a maintainer can register them next to the other 8 passes
// (Renderer.cpp:577-585) and call RecordCommands() where the D3D12 code recorded command lists. "Recording" here means
// enqueueing HIP kernels on a stream through the C ABI (include/vqhip.h); nothing else is linked.
// Passes that are one C call and have no adaptor class here:
//     ResolveMSAA_DepthPrePass + DownsampleDepth   SceneRendering.cpp:484-499 -> vqhip_msaa_resolve_surfaces(.., hierarchy, flags): resolve + the whole depth chain
//     DownsampleDepth alone (MSAA off, :491-499)   -> vqhip_depth_hierarchy
// Header-only, C++17, needs the HIP runtime only for buffer allocation (hipMalloc/hipFree).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <string>
#include <vector>
#include "vqhip.h"

// The interface the adaptors derive from:
//   * inside the engine: define VQHIP_ENGINE_RENDERPASS_H to the include path of the engine's own RenderPass.h (e.g.
//     -DVQHIP_ENGINE_RENDERPASS_H='"Renderer/Rendering/RenderPass/RenderPass.h"'). The adaptors then derive from the ENGINE'S ::IRenderPass,
//     implement its CollectPSOCreationParameters() (RenderPass.h:58) as "no PSOs: kernels are compiled ahead of time", and can be stored
//     in VQRenderer::mRenderPasses (std::vector<std::shared_ptr<IRenderPass>>, Renderer.h:403) next to the other passes;
//   * stand-alone (tests, tools): the stand-in interface below with the same five virtuals.
// tests/cpp/test_passes_engine.cpp compiles the first form against a stand-in of the engine header (tests/cpp/mock_engine/).
#ifdef VQHIP_ENGINE_RENDERPASS_H
#include VQHIP_ENGINE_RENDERPASS_H
namespace vqhip {
using IRenderPassResourceCollection = ::IRenderPassResourceCollection;      // RenderPass.h:27
using IRenderPassDrawParameters = ::IRenderPassDrawParameters;              // RenderPass.h:29
class IRenderPass : public ::IRenderPass {                                  // RenderPass.h:44-59
public:
    std::vector<FPSOCreationTaskParameters> CollectPSOCreationParameters() override { return {}; }   // :58 — nothing to compile at load time
    int LastStatus() const { return mStatus; }      // the reference asserts/logs; here the last vqhip_status is kept
protected:
    int mStatus = VQHIP_OK;
};
} // namespace vqhip
#else
namespace vqhip {
struct IRenderPassResourceCollection {};            // RenderPass.h:27
struct IRenderPassDrawParameters {};                // RenderPass.h:29

class IRenderPass {                                 // RenderPass.h:44-59 (CollectPSOCreationParameters only exists in the engine build above)
public:
    virtual ~IRenderPass() = default;
    virtual bool Initialize() = 0;
    virtual void Destroy() = 0;
    virtual void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* pRscParameters = nullptr) = 0;
    virtual void OnDestroyWindowSizeDependentResources() = 0;
    virtual void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) = 0;
    int LastStatus() const { return mStatus; }      // the reference asserts/logs; here the last vqhip_status is kept
protected:
    int mStatus = VQHIP_OK;
};
} // namespace vqhip
#endif

namespace vqhip {

class RenderPassBase : public IRenderPass {         // RenderPass.h:65-89: holds the renderer; here the vqhip context
protected:
    explicit RenderPassBase(vqhip_ctx* Ctx) : mCtx(Ctx) {}
    vqhip_ctx* mCtx;
    static void* Alloc(size_t bytes) { void* p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
    static void Free(void*& p) { if (p) { (void)hipFree(p); p = nullptr; } }
    // A device buffer a pass owns and sizes on demand (the library itself never allocates). Reserve refuses need == 0, keeps a buffer that is large enough and
    // otherwise frees the old one before it allocates (hipFree waits for the device); the buffer only grows. Freed with the pass.
    struct WorkBuffer {
        void* ptr = nullptr; size_t bytes = 0;
        WorkBuffer() = default;
        WorkBuffer(const WorkBuffer&) = delete;
        WorkBuffer& operator=(const WorkBuffer&) = delete;
        ~WorkBuffer() { Release(); }
        bool Reserve(size_t need) {
            if (!need) return false;
            if (need <= bytes) return true;
            Release();
            ptr = Alloc(need);
            if (ptr) bytes = need;
            return ptr != nullptr;
        }
        void Release() { Free(ptr); bytes = 0; }
    };
    template <class DRAW> static uint64_t InstancedTriangles(const DRAW& d) { return (uint64_t)(d.mesh.numIndices / 3) * d.numInstances; }
};

// A pass that owns no resource, window-sized or other: the caller brings every plane with the draw parameters.
class OwnsNothingPass : public RenderPassBase {
public:
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override {}
    void OnCreateWindowSizeDependentResources(unsigned, unsigned, const IRenderPassResourceCollection* = nullptr) override {}
    void OnDestroyWindowSizeDependentResources() override {}
protected:
    using RenderPassBase::RenderPassBase;
};

// ---------------------------------------------------------------------------------------------------------------
// Forward lighting == VQRenderer::RenderSceneColor (SceneRendering.cpp:1619-1851, lit draws :1730-1784).
// Owns the scene-colour target (Tex_SceneColor, RGBA16F: RenderResources.cpp:40,144-161).
// ---------------------------------------------------------------------------------------------------------------
class HipForwardLightingPass : public RenderPassBase {
public:
    struct FResourceCollection : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;                                  // replaces ID3D12GraphicsCommandList* pCmd
        vqhip_gbuffer GBuffer = {};                              // replaces the rasterised PSInput + material textures
        // Alternative input: rasteriser output + materials; when pInterpolants != nullptr the pass first runs
        // vqhip_gbuffer_from_materials (PSMain :226-287) into its own G-buffer planes and GBuffer above is ignored.
        const vqhip_interpolants* pInterpolants = nullptr;
        const vqhip_material* pMaterials = nullptr;              // cbPerObject.materialData + SRV tables of every material on screen
        int NumMaterials = 0;
        const vqhip_ssao* pScreenSpaceAO = nullptr;              // Tex_AmbientOcclusion or nullptr (SSAO off)
        const VQ_PerFrameData* pPerFrame = nullptr;              // == cbPerFrame  (SceneRendering.cpp:429-450)
        const VQ_PerViewLightingData* pPerView = nullptr;        // == cbPerView   (:452-467)
        const VQ_PointLight* pExtraPointLights = nullptr;        // extension: lights beyond NUM_LIGHTS__POINT
        int NumExtraPointLights = 0;
        const vqhip_envmap* pEnvironmentMap = nullptr;           // nullptr == bDrawEnvironmentMap false (NullCubemapSRV, :1698-1709)
        const vqhip_shadowmaps* pShadowMaps = nullptr;
        // the draw's other render targets (SceneRendering.cpp:1640-1641,1662-1663 -> PSO permutations OUTPUT_ALBEDO / OUTPUT_MOTION_VECTORS)
        bool bUseVisualizationRenderTarget = false;              // SV_TARGET1 = (albedo, metalness) into Tex_SceneVisualization (RGBA16F)
        bool bRenderMotionVectors = false;                       // motion vectors into Tex_SceneMotionVectors (RG16F); needs the two planes below
        const void* pSvPositionCurr = nullptr;                   // PSInput.svPositionCurr / svPositionPrev (ForwardLighting.hlsl:49-52): float4 per pixel, tightly packed
        const void* pSvPositionPrev = nullptr;
    };
    explicit HipForwardLightingPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~HipForwardLightingPass() override { OnDestroyWindowSizeDependentResources(); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { OnDestroyWindowSizeDependentResources(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override {
        OnDestroyWindowSizeDependentResources();
        mWidth = Width; mHeight = Height;
        mSceneColor = Alloc((size_t)Width * Height * 8);
    }
    void OnDestroyWindowSizeDependentResources() override {
        Free(mSceneColor); Free(mSceneVisualization); Free(mSceneMotionVectors);
        for (void*& g : mGB) Free(g);
        mWidth = mHeight = 0;
    }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !mSceneColor) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        vqhip_gbuffer gb = p->GBuffer;
        if (p->pInterpolants) {
            if (!p->pPerFrame) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
            for (void*& g : mGB) if (!g) g = Alloc((size_t)mWidth * mHeight * 16);     // planes allocated on first use
            gb = { mGB[0], mGB[1], mGB[2], mGB[3], (int32_t)mWidth, (int32_t)mHeight, (int32_t)mWidth };
            mStatus = vqhip_gbuffer_from_materials(mCtx, p->Stream, p->pInterpolants, p->pMaterials, p->NumMaterials,
                                                   p->pPerFrame->fAmbientLightingFactor, p->pScreenSpaceAO, &gb);
            if (mStatus != VQHIP_OK) return;
        }
        vqhip_psmain_targets t = {};
        if (p->bUseVisualizationRenderTarget) {
            if (!mSceneVisualization) mSceneVisualization = Alloc((size_t)mWidth * mHeight * 8);
            t.albedo_metallic = mSceneVisualization; t.albedo_fmt = VQHIP_FMT_RGBA16F;
        }
        if (p->bRenderMotionVectors) {
            if (!mSceneMotionVectors) mSceneMotionVectors = Alloc((size_t)mWidth * mHeight * 4);
            t.motion_vectors = mSceneMotionVectors; t.motion_fmt = VQHIP_FMT_RG16F;
            t.svPositionCurr = p->pSvPositionCurr; t.svPositionPrev = p->pSvPositionPrev;
        }
        mStatus = vqhip_forward_lighting_mrt(mCtx, p->Stream, &gb, p->pPerFrame, p->pPerView, p->pExtraPointLights, p->NumExtraPointLights,
                                             p->pEnvironmentMap, p->pShadowMaps, mSceneColor, (int)mWidth, VQHIP_FMT_RGBA16F, &t);
    }
    void* GetSceneColor() const { return mSceneColor; }          // RGBA16F, width*height
    void* GetSceneVisualization() const { return mSceneVisualization; }   // RGBA16F (albedo, metalness); nullptr until a draw asked for it
    void* GetSceneMotionVectors() const { return mSceneMotionVectors; }   // RG16F; nullptr until a draw asked for it
    unsigned Width() const { return mWidth; }
    unsigned Height() const { return mHeight; }
private:
    void* mSceneColor = nullptr;
    void* mSceneVisualization = nullptr;                         // Tex_SceneVisualization (RenderResources.cpp:171-175)
    void* mSceneMotionVectors = nullptr;                         // Tex_SceneMotionVectors (RenderResources.cpp:178-182)
    void* mGB[4] = { nullptr, nullptr, nullptr, nullptr };       // G-buffer planes of the §8f.1 producer path
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Post-process == VQRenderer::RenderPostProcess (SceneRendering.cpp:2507-2788): [blur X,Y :2582-2638] -> tonemapper :2640-2656.
// Owns BlurIntermediate / BlurOutput (RGBA16F, RenderResources.cpp:221-243) and TonemapperOut (RGBA8 SDR / RGBA16F HDR, :245-261).
// Returns the buffer holding the final image like the reference returns ID3D12Resource*.
// ---------------------------------------------------------------------------------------------------------------
class HipPostProcessPass : public RenderPassBase {
public:
    struct FResourceCollection : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const void* pSceneColor = nullptr;                       // RGBA16F input (HipForwardLightingPass::GetSceneColor())
        VQ_TonemapperParams TonemapperParams = { VQ_COLOR_SPACE_REC_709, VQ_DISPLAY_CURVE_SRGB, 200.0f, 1 };   // FTonemapper defaults, PostProcess.h:84-91
        bool bEnableGaussianBlur = false;                        // FPostProcessParameters::bEnableGaussianBlur (PostProcess.h:166); compiled out in the reference (:2526)
        bool bHDR = false;                                       // selects the RGBA16F tonemapper target
        // Row-tiled multi-GPU frame (no reference analogue): this pass was sized for ONE ROW TILE of the frame
        // (vqhip_rowtile) and pSceneColor is that tile. With pComm set the pass exchanges 10 halo rows with the tiles above / below — rows of SCENE COLOUR right
        // behind the shade kernel on the SDR path (one call filters X, Y and tonemaps), X-blurred rows before the Y blur on the HDR path — and afterwards
        // composites the finished tiles into pCompositeFrame on CompositeRoot
        // (VQHIP_ALL_RANKS: on every rank). pCompositeFrame: FrameHeight x Width texels of the output format, or nullptr on ranks that
        // do not receive the frame.
        vqhip_comm* pComm = nullptr;                             // its size and this process's rank are read from it (vqhip_comm_query)
        int FrameHeight = 0;
        int CompositeRoot = 0;
        void* pCompositeFrame = nullptr;
    };
    explicit HipPostProcessPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~HipPostProcessPass() override { OnDestroyWindowSizeDependentResources(); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { OnDestroyWindowSizeDependentResources(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override {
        OnDestroyWindowSizeDependentResources();
        mWidth = Width; mHeight = Height;
        const size_t px = (size_t)Width * Height;
        mTonemapperOut = Alloc(px * 8);                          // BlurIntermediate / BlurOutput (16 B/px) are allocated on first use of the HDR path only: the SDR path
                                                                 // never touches them (one kernel for frames of >= 2^20 pixels; below that, or for a curve that mixes channels,
                                                                 // vqhip_post_process_tile blurs into the CONTEXT's scratch buffer — one more reason why a context
                                                                 // serves one thread and one stream at a time)
        mHaloTop = Alloc((size_t)VQHIP_HALO_ROWS * Width * 8); mHaloBottom = Alloc((size_t)VQHIP_HALO_ROWS * Width * 8);   // row-tiled mode only
    }
    void OnDestroyWindowSizeDependentResources() override {
        Free(mBlurIntermediate); Free(mBlurOutput); Free(mTonemapperOut); Free(mHaloTop); Free(mHaloBottom); mWidth = mHeight = 0;
        mBlurIntermediate = mBlurOutput = mTonemapperOut = mHaloTop = mHaloBottom = nullptr;
    }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !p->pSceneColor || !mTonemapperOut) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mOutFormat = p->bHDR ? VQHIP_FMT_RGBA16F : VQHIP_FMT_RGBA8_UNORM;
        // Row-tiled mode: size and rank come from the communicator itself, and the tile geometry is validated BEFORE anything is enqueued on
        // it — a rank that fails here has not posted a send its neighbours would wait for.
        int world = 1, rank = 0;
        if (p->pComm) {
            vqhip_comm_info info;
            mStatus = vqhip_comm_query(p->pComm, &info);
            if (mStatus != VQHIP_OK) return;
            world = info.world; rank = info.rank;
            int row0 = 0, rows = 0;
            mStatus = vqhip_rowtile(p->FrameHeight, world, rank, &row0, &rows);
            if (mStatus == VQHIP_OK && rows != (int)mHeight) mStatus = VQHIP_ERR_INVALID_ARG;                 // the pass must have been sized for this tile
            if (mStatus == VQHIP_OK && (p->CompositeRoot == VQHIP_ALL_RANKS || p->CompositeRoot == rank) && !p->pCompositeFrame) mStatus = VQHIP_ERR_INVALID_ARG;
            if (mStatus != VQHIP_OK) return;
        }
        if (p->bEnableGaussianBlur && !p->bHDR) {
            // SDR: CSMain_X, CSMain_Y and the tonemapper (SceneRendering.cpp:2582-2656) are ONE call — one kernel for frames of >= 2^20 pixels (neither BlurIntermediate
            // nor BlurOutput touches HBM), identical bits to the separate dispatches. Row-tiled mode: exchange 1 moves the 10 boundary rows of SCENE COLOUR right behind
            // the shade kernel (the X pass is horizontal: the neighbour's rows are filtered here like the tile's own).
            const void* top = nullptr; const void* bottom = nullptr; int haloRows = 0;
            if (p->pComm) {
                mStatus = vqhip_exchange_blur_halos(p->pComm, p->Stream, p->pSceneColor, (int)mWidth, (int)mHeight, (int)mWidth, VQHIP_FMT_RGBA16F, mHaloTop, mHaloBottom);
                if (mStatus != VQHIP_OK) return;
                top = rank > 0 ? mHaloTop : nullptr; bottom = rank < world - 1 ? mHaloBottom : nullptr; haloRows = (top || bottom) ? VQHIP_HALO_ROWS : 0;
            }
            mStatus = vqhip_post_process_tile(mCtx, p->Stream, p->pSceneColor, mTonemapperOut, top, bottom, haloRows, (int)mWidth, (int)mHeight, &p->TonemapperParams,
                                              VQHIP_FMT_RGBA16F, mOutFormat);
        } else if (p->bEnableGaussianBlur) {
            // HDR (RGBA16F out): CSMain_X -> BlurIntermediate, CSMain_Y -> BlurOutput, tonemapper — the fused Y + tonemap kernel on the LDS tile is slower than two
            // dispatches there, so it keeps them.
            const VQ_BlurParams bp = { (int32_t)mWidth, (int32_t)mHeight };                                      // FBlurParams, PostProcess.h:92-96
            if (!mBlurIntermediate) { const size_t px = (size_t)mWidth * mHeight; mBlurIntermediate = Alloc(px * 8); mBlurOutput = Alloc(px * 8); }
            if (!mBlurIntermediate || !mBlurOutput) { mStatus = VQHIP_ERR_HIP; return; }
            mStatus = vqhip_gaussian_blur_x(mCtx, p->Stream, p->pSceneColor, mBlurIntermediate, &bp, VQHIP_FMT_RGBA16F);
            if (mStatus != VQHIP_OK) return;
            const void* top = nullptr; const void* bottom = nullptr; int haloRows = 0;
            if (p->pComm) {                                      // exchange 1: the 10 boundary rows of the X-blurred tile (RCCL send/recv on p->Stream)
                mStatus = vqhip_exchange_blur_halos(p->pComm, p->Stream, mBlurIntermediate, (int)mWidth, (int)mHeight, (int)mWidth, VQHIP_FMT_RGBA16F, mHaloTop, mHaloBottom);
                if (mStatus != VQHIP_OK) return;
                top = rank > 0 ? mHaloTop : nullptr; bottom = rank < world - 1 ? mHaloBottom : nullptr; haloRows = (top || bottom) ? VQHIP_HALO_ROWS : 0;
            }
            mStatus = vqhip_gaussian_blur_y(mCtx, p->Stream, mBlurIntermediate, mBlurOutput, top, bottom, haloRows, &bp, VQHIP_FMT_RGBA16F);
            if (mStatus != VQHIP_OK) return;
            mStatus = vqhip_tonemap(mCtx, p->Stream, mBlurOutput, mTonemapperOut, (int)mWidth, (int)mHeight, &p->TonemapperParams, VQHIP_FMT_RGBA16F, mOutFormat);
        } else {
            mStatus = vqhip_tonemap(mCtx, p->Stream, p->pSceneColor, mTonemapperOut, (int)mWidth, (int)mHeight, &p->TonemapperParams, VQHIP_FMT_RGBA16F, mOutFormat);
        }
        if (mStatus == VQHIP_OK && p->pComm)                     // exchange 2: the finished tiles -> the frame on the presenting rank
            mStatus = vqhip_composite_tiles(p->pComm, p->Stream, mTonemapperOut, (int)mWidth, p->FrameHeight, mOutFormat, p->CompositeRoot, p->pCompositeFrame);
    }
    void* GetOutput() const { return mTonemapperOut; }
    vqhip_format GetOutputFormat() const { return mOutFormat; }
private:
    void* mHaloTop = nullptr; void* mHaloBottom = nullptr;
    void* mBlurIntermediate = nullptr; void* mBlurOutput = nullptr; void* mTonemapperOut = nullptr;
    vqhip_format mOutFormat = VQHIP_FMT_RGBA8_UNORM;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Environment-map prefilter == FEnvironmentMapRenderingResources::CreateRenderingResources (EnvironmentMapRendering.cpp:20-106)
// + VQRenderer::PreFilterEnvironmentMap (:139-486) + ComputeBRDFIntegrationLUT (Renderer.cpp:871-909).
// "Window size" plays no role; resources depend on the HDRI and the two resolutions.
// ---------------------------------------------------------------------------------------------------------------
class HipEnvMapPrefilterPass : public RenderPassBase {
public:
    struct FResourceCollection : public IRenderPassResourceCollection {
        int DiffuseIrradianceCubemapResolution = 64;             // EnvironmentMap.cpp:214
        int SpecularMapMip0Resolution = 128;                     // gfx.EnvironmentMapResolution (Settings.h:48)
        int HDRIWidth = 0, HDRIHeight = 0;
    };
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const void* pEquirectRGBA32F = nullptr;                  // device, HDRIWidth x HDRIHeight float4 (level 0 only; mips are generated here)
        float DiffuseIntegrationStep = 0.010f;                   // INTEGRATION_STEP_DIFFUSE_IRRADIANCE, PipelineStateObjects.cpp:1298-1306
        vqhip_conv_order Order = VQHIP_CONV_SEQUENTIAL;                // the reference's summation order (CubemapConvolution.hlsl:132-163,186-219)
        bool bComputeBRDFLUT = true;                             // LoadDefaultResources does this once (Renderer.cpp:934)
    };
    explicit HipEnvMapPrefilterPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~HipEnvMapPrefilterPass() override { DestroyRenderingResources(); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { DestroyRenderingResources(); }
    void OnCreateWindowSizeDependentResources(unsigned, unsigned, const IRenderPassResourceCollection* pRsc = nullptr) override {
        const FResourceCollection* r = static_cast<const FResourceCollection*>(pRsc);
        if (!r) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        DestroyRenderingResources();
        mRsc = *r;
        mNumMips = vqhip_mip_level_count(r->HDRIWidth, r->HDRIHeight);
        mSpecMips = vqhip_specular_mip_count(r->SpecularMapMip0Resolution);
        const size_t face = (size_t)r->DiffuseIrradianceCubemapResolution * r->DiffuseIrradianceCubemapResolution * 8;
        mChain = Alloc(vqhip_mip_chain_bytes(r->HDRIWidth, r->HDRIHeight, mNumMips));
        mDiff = Alloc(6 * face); mDiffBlurred = Alloc(6 * face); mBlurTemp = Alloc(face);
        mSpec = Alloc(vqhip_cube_bytes(r->SpecularMapMip0Resolution, mSpecMips, VQHIP_FMT_RGBA16F));
        mLUT = Alloc((size_t)1024 * 1024 * 4);                   // 1024^2 RG16F, Renderer.cpp:1026-1032
    }
    void OnDestroyWindowSizeDependentResources() override { DestroyRenderingResources(); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !p->pEquirectRGBA32F || !mChain) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        const size_t l0 = (size_t)mRsc.HDRIWidth * mRsc.HDRIHeight * 16;
        if (hipMemcpyAsync(mChain, p->pEquirectRGBA32F, l0, hipMemcpyDeviceToDevice, (hipStream_t)p->Stream) != hipSuccess) { mStatus = VQHIP_ERR_HIP; return; }
        mStatus = vqhip_mip_chain_min_rgba32f(mCtx, p->Stream, mChain, mRsc.HDRIWidth, mRsc.HDRIHeight, mNumMips);   // TextureManager.cpp:590-592,643-738
        if (mStatus != VQHIP_OK) return;
        const vqhip_envmap_out out = { mDiff, mDiffBlurred, mBlurTemp, mSpec };
        mStatus = vqhip_envmap_prefilter(mCtx, p->Stream, mChain, mRsc.HDRIWidth, mRsc.HDRIHeight, mNumMips, mRsc.DiffuseIrradianceCubemapResolution,
                                         p->DiffuseIntegrationStep, mRsc.SpecularMapMip0Resolution, p->Order, &out);
        if (mStatus != VQHIP_OK || !p->bComputeBRDFLUT) return;
        mStatus = vqhip_brdf_lut(mCtx, p->Stream, mLUT, 1024, 2048, VQHIP_FMT_RG16F);                             // Renderer.cpp:895-900
    }
    // what RenderSceneColor binds at SceneRendering.cpp:1698-1709
    vqhip_envmap GetEnvironmentMap() const { return vqhip_envmap{ mDiffBlurred, mRsc.DiffuseIrradianceCubemapResolution, mSpec, mRsc.SpecularMapMip0Resolution, mSpecMips, mLUT, 1024 }; }
    int GetNumSpecularIrradianceCubemapLODLevels() const { return mSpecMips; }   // -> PerViewLightingData::MaxEnvMapLODLevels (SceneRendering.cpp:463)
private:
    void DestroyRenderingResources() { Free(mChain); Free(mDiff); Free(mDiffBlurred); Free(mBlurTemp); Free(mSpec); Free(mLUT); }   // :108
    FResourceCollection mRsc;
    int mNumMips = 0, mSpecMips = 0;
    void* mChain = nullptr; void* mDiff = nullptr; void* mDiffBlurred = nullptr; void* mBlurTemp = nullptr; void* mSpec = nullptr; void* mLUT = nullptr;
};

// ---------------------------------------------------------------------------------------------------------------
// SSR environment fallback == the part of ScreenSpaceReflectionsPass::RecordCommands' "FFX DNSR ClassifyTiles" dispatch
// (ScreenSpaceReflections.cpp:262-276) that consumes the specular cube + BRDF LUT: pixels too rough for a traced ray get
// SampleEnvironmentMap (ClassifyReflectionTiles.hlsl:78-94,146-153). FResourceParameters / FDrawParameters keep the fields of
// ScreenSpaceReflections.h:33-75 this part reads (textures as device pointers, SRVs as the vqhip_envmap). Owns TexRadiance
// (RGBA16F, :129) and TexExtractedRoughness (R8_UNORM, :135); the radiance is what vqhip_apply_reflections adds to the scene colour
// when no ray was traced; HipSSRIntersectPass below traces the rays into the same TexRadiance (the reflection denoiser: out of scope).
// ---------------------------------------------------------------------------------------------------------------
class HipSSREnvironmentFallbackPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        VQ_SSSRConstants ffxCBuffer = {};                        // == FDrawParameters::ffxCBuffer, filled as RenderReflections does (SceneRendering.cpp:2221-2242)
        const void* TexSceneColorRoughness = nullptr;            // RGBA16F scene colour, alpha = roughness (HipForwardLightingPass::GetSceneColor())
        const float* TexDepthHierarchy = nullptr;                // mip 0 of Tex_DownsampledSceneDepth, R32F
        const void* TexNormals = nullptr;                        // Tex_SceneNormals, R10G10B10A2_UNORM
        const vqhip_envmap* SRVEnvironmentSpecularIrradianceCubemap_BRDFIntegrationLUT = nullptr;   // the two SRVs of :268-269 (HipEnvMapPrefilterPass::GetEnvironmentMap())
    };
    explicit HipSSREnvironmentFallbackPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~HipSSREnvironmentFallbackPass() override { OnDestroyWindowSizeDependentResources(); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { OnDestroyWindowSizeDependentResources(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override {
        OnDestroyWindowSizeDependentResources();
        mWidth = Width; mHeight = Height;
        mRadiance = Alloc((size_t)Width * Height * 8); mExtractedRoughness = Alloc((size_t)Width * Height);
    }
    void OnDestroyWindowSizeDependentResources() override { Free(mRadiance); Free(mExtractedRoughness); mWidth = mHeight = 0; }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !mRadiance) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mStatus = vqhip_ssr_environment_fallback(mCtx, p->Stream, p->TexSceneColorRoughness, VQHIP_FMT_RGBA16F, 0, p->TexDepthHierarchy, 0,
                                                 p->TexNormals, VQHIP_FMT_R10G10B10A2_UNORM, 0, (int)mWidth, (int)mHeight, &p->ffxCBuffer,
                                                 p->SRVEnvironmentSpecularIrradianceCubemap_BRDFIntegrationLUT, mRadiance, VQHIP_FMT_RGBA16F, 0, (uint8_t*)mExtractedRoughness);
    }
    void* GetRadiance() const { return mRadiance; }                      // RGBA16F
    void* GetExtractedRoughness() const { return mExtractedRoughness; }  // R8_UNORM
private:
    void* mRadiance = nullptr; void* mExtractedRoughness = nullptr;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// SSR rays == the ray list of the "FFX DNSR ClassifyTiles" dispatch + the "FFX SSSR Intersection" dispatch of
// ScreenSpaceReflectionsPass::RecordCommands (ScreenSpaceReflections.cpp:262-320): vqhip_ssr_classify + vqhip_ssr_intersect. Owns TexRayList,
// TexRayCounter and TexDenoiserTileList (ScreenSpaceReflections.cpp:118-127, as plain device buffers); traces IN PLACE into the TexRadiance that
// HipSSREnvironmentFallbackPass owns and has filled on the same stream. Without the denoiser passes behind it (HipSSRReprojectPass / HipSSRPrefilterPass / HipSSRResolveTemporalPass below), run it with ffxCBuffer.samplesPerQuad = 4: every
// glossy pixel then traces its own ray and the radiance is directly what vqhip_composite_reflections consumes.
// ---------------------------------------------------------------------------------------------------------------
class HipSSRIntersectPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        VQ_SSSRConstants ffxCBuffer = {};                        // the same block HipSSREnvironmentFallbackPass gets
        const void* TexSceneColorRoughness = nullptr;            // g_roughness (classify) and g_lit_scene (intersect): the RGBA16F scene colour, alpha = roughness
        const float* TexDepthHierarchy = nullptr;                // ALL levels of Tex_DownsampledSceneDepth: the buffer of vqhip_depth_hierarchy / vqhip_msaa_resolve_surfaces
        const void* TexNormals = nullptr;                        // Tex_SceneNormals, R10G10B10A2_UNORM
        const void* TexVarianceHistory = nullptr;                // R16F, or nullptr (reads 0)
        const uint8_t* TexExtractedRoughness = nullptr;          // HipSSREnvironmentFallbackPass::GetExtractedRoughness()
        const uint8_t* TexBlueNoise = nullptr;                   // 128 x 128 R8G8_UNORM (the engine's PrepareBlueNoiseTexture output)
        void* TexRadiance = nullptr;                             // HipSSREnvironmentFallbackPass::GetRadiance(), RGBA16F
        const vqhip_envmap* SRVEnvironmentSpecularIrradianceCubemap_BRDFIntegrationLUT = nullptr;
    };
    explicit HipSSRIntersectPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~HipSSRIntersectPass() override { OnDestroyWindowSizeDependentResources(); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { OnDestroyWindowSizeDependentResources(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override {
        OnDestroyWindowSizeDependentResources();
        mWidth = Width; mHeight = Height;
        mRayList = Alloc((size_t)Width * Height * 4); mRayCounter = Alloc(2 * 4);
        mDenoiserTileList = Alloc((size_t)((Width + 7) / 8) * ((Height + 7) / 8) * 4);
    }
    void OnDestroyWindowSizeDependentResources() override { Free(mRayList); Free(mRayCounter); Free(mDenoiserTileList); mWidth = mHeight = 0; }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !mRayList || p->ffxCBuffer.bufferDimensions[0] != mWidth || p->ffxCBuffer.bufferDimensions[1] != mHeight) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mStatus = vqhip_ssr_classify(mCtx, p->Stream, p->TexSceneColorRoughness, VQHIP_FMT_RGBA16F, 0, p->TexDepthHierarchy, 0, p->TexVarianceHistory, 0,
                                     &p->ffxCBuffer, (uint32_t*)mRayList, (uint32_t*)mRayCounter, (uint32_t*)mDenoiserTileList);
        if (mStatus != VQHIP_OK) return;
        mStatus = vqhip_ssr_intersect(mCtx, p->Stream, (const uint32_t*)mRayList, (const uint32_t*)mRayCounter, p->TexSceneColorRoughness, VQHIP_FMT_RGBA16F, 0,
                                      p->TexDepthHierarchy, p->TexNormals, VQHIP_FMT_R10G10B10A2_UNORM, 0, p->TexExtractedRoughness, p->TexBlueNoise, &p->ffxCBuffer,
                                      p->SRVEnvironmentSpecularIrradianceCubemap_BRDFIntegrationLUT, p->TexRadiance, VQHIP_FMT_RGBA16F, 0);
    }
    const uint32_t* GetRayList() const { return (const uint32_t*)mRayList; }                  // PackRayCoords words, device
    const uint32_t* GetRayCounter() const { return (const uint32_t*)mRayCounter; }            // { rays, denoiser tiles }, device
    const uint32_t* GetDenoiserTileList() const { return (const uint32_t*)mDenoiserTileList; }
private:
    void* mRayList = nullptr; void* mRayCounter = nullptr; void* mDenoiserTileList = nullptr;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Ambient occlusion == AmbientOcclusionPass::RecordCommands -> FFX_CACAO_D3D12Draw (AmbientOcclusion.cpp; VQRenderer::RenderAmbientOcclusion,
// SceneRendering.cpp:1503-1555): vqhip_cacao at quality HIGH, native resolution. Owns FidelityFX CACAO's intermediates (the deinterleaved depths and
// normals, the ping / pong occlusion planes) as ONE work buffer, sized for the window like FFX_CACAO_D3D12InitScreenSizeDependentResources does. The
// engine keeps filling the constants with FidelityFX's own FFX_CACAO_UpdateBufferSizeInfo / _UpdateConstants / _UpdatePerPassConstants from
// FDrawParameters::matProj / matNormalToView and hands the five blocks over; TexAmbientOcclusion is what the lit draw reads as texScreenSpaceAO.
// ---------------------------------------------------------------------------------------------------------------
class AmbientOcclusionPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        VQ_CacaoConstants Constants = {};                        // FFX_CACAO_UpdateConstants
        VQ_CacaoConstants PerPassConstants[4] = {};              // + FFX_CACAO_UpdatePerPassConstants(.., i)
        int BlurPassCount = 2;                                   // FFX_CACAO_Settings::blurPassCount
        const float* TexSceneDepthResolve = nullptr;             // Tex_SceneDepthResolve, R32F, dense rows
        const void* TexSceneNormals = nullptr;                   // Tex_SceneNormals, R10G10B10A2_UNORM, dense rows
        uint8_t* TexAmbientOcclusion = nullptr;                  // Tex_AmbientOcclusion, R8_UNORM, dense rows
    };
    explicit AmbientOcclusionPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~AmbientOcclusionPass() override { OnDestroyWindowSizeDependentResources(); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { OnDestroyWindowSizeDependentResources(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override {
        OnDestroyWindowSizeDependentResources();
        mWidth = Width; mHeight = Height;
        mWork.Reserve(vqhip_cacao_work_bytes((int)Width, (int)Height));
    }
    void OnDestroyWindowSizeDependentResources() override { mWork.Release(); mWidth = mHeight = 0; }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !mWork.ptr) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mStatus = vqhip_cacao(mCtx, p->Stream, p->TexSceneDepthResolve, (size_t)mWidth * 4, p->TexSceneNormals, VQHIP_FMT_R10G10B10A2_UNORM, (size_t)mWidth * 4,
                              &p->Constants, p->PerPassConstants, VQHIP_CACAO_QUALITY_HIGH, p->BlurPassCount, mWork.ptr, mWork.bytes, p->TexAmbientOcclusion,
                              (size_t)mWidth, (int)mWidth, (int)mHeight);
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }      // vqhip_cacao_plane_offset_bytes addresses the intermediates
private:
    WorkBuffer mWork;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Ambient occlusion at FFX_CACAO_DEFAULT_SETTINGS' own quality, HIGHEST — what AmbientOcclusionPass's constructor sets (AmbientOcclusion.cpp:38):
// vqhip_adaptive_cacao. The same parameters and the same roles as AmbientOcclusionPass above; the work buffer is the larger one of
// vqhip_adaptive_cacao_work_bytes (HIGH's layout, then the importance map, its pong and the load counter). The constants come from FidelityFX's own functions with
// settings.qualityLevel = FFX_CACAO_QUALITY_HIGHEST: LoadCounterAvgDiv, AdaptiveSampleCountLimit and ImportanceMapDimensions are read here.
// ---------------------------------------------------------------------------------------------------------------
class AdaptiveAmbientOcclusionPass : public RenderPassBase {
public:
    using FResourceParameters = AmbientOcclusionPass::FResourceParameters;
    using FDrawParameters = AmbientOcclusionPass::FDrawParameters;
    explicit AdaptiveAmbientOcclusionPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~AdaptiveAmbientOcclusionPass() override { OnDestroyWindowSizeDependentResources(); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { OnDestroyWindowSizeDependentResources(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override {
        OnDestroyWindowSizeDependentResources();
        mWidth = Width; mHeight = Height;
        mWork.Reserve(vqhip_adaptive_cacao_work_bytes((int)Width, (int)Height));
    }
    void OnDestroyWindowSizeDependentResources() override { mWork.Release(); mWidth = mHeight = 0; }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !mWork.ptr) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mStatus = vqhip_adaptive_cacao(mCtx, p->Stream, p->TexSceneDepthResolve, (size_t)mWidth * 4, p->TexSceneNormals, VQHIP_FMT_R10G10B10A2_UNORM, (size_t)mWidth * 4,
                                       &p->Constants, p->PerPassConstants, p->BlurPassCount, mWork.ptr, mWork.bytes, p->TexAmbientOcclusion,
                                       (size_t)mWidth, (int)mWidth, (int)mHeight);
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }      // vqhip_adaptive_cacao_plane_offset_bytes addresses the intermediates
private:
    WorkBuffer mWork;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Shadow maps == VQRenderer::RenderDirectionalShadowMaps + RenderSpotShadowMaps + RenderPointShadowMaps (SceneRendering.cpp:1114-1263) with
// DrawShadowViewMeshList (:996-1040): vqhip_shadow_depth, every view of the frame in ONE call. FDrawParameters carries what the three functions hold per view:
// the draw lists (FSceneDrawData::directionalShadowDrawParams / spotShadowDrawParams[i] / pointShadowDrawParams[i * 6 + face], each FInstancedDrawParameters as a
// vqhip_shadow_draw whose matrices are the uploaded PerObjectShadowData), the casters' position and range (SetPerViewShadowCB) and the three depth arrays the lit
// draw reads through vqhip_shadowmaps (DSV_ShadowMaps_Directional / _Spot / _Point as R32F). As in the engine, a view whose draw list is empty is skipped: its
// map is neither cleared nor drawn. Point faces are LINEAR_DEPTH (iDepthMode 1), the others z/w. The pass owns the work buffer: Reserve sizes it for a triangle
// count ahead of time; RecordCommands grows it when a frame needs more (hipFree of the old buffer waits for the device; the library itself never allocates).
// ---------------------------------------------------------------------------------------------------------------
class ShadowDepthPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        float* ShadowMapsDirectional = nullptr; int DirectionalDim = 2048;      // [dim][dim]                     SceneRendering.cpp:1128
        float* ShadowMapsSpot = nullptr;        int SpotDim = 1024;             // [NumSpotShadowViews][dim][dim] :1166
        float* ShadowMapsPoint = nullptr;       int PointDim = 1024;            // [NumPointShadowViews][6][dim][dim] :1219
        const std::vector<vqhip_shadow_draw>* DirectionalDraws = nullptr;       // nullptr or empty: the directional map is skipped (:1122)
        unsigned NumSpotShadowViews = 0;
        const std::vector<vqhip_shadow_draw>* SpotDraws[VQ_NUM_SHADOWING_LIGHTS__SPOT] = {};
        unsigned NumPointShadowViews = 0;                                       // point LIGHTS; six views each
        const std::vector<vqhip_shadow_draw>* PointDraws[VQ_NUM_SHADOWING_LIGHTS__POINT * 6] = {};
        VQ_float3 PointPosition[VQ_NUM_SHADOWING_LIGHTS__POINT] = {};           // GPULightingData.point_casters[i].position (:1234)
        float PointRange[VQ_NUM_SHADOWING_LIGHTS__POINT] = {};                  // ... .range, the far plane (:1235)
    };
    explicit ShadowDepthPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { mWork.Release(); }
    void OnCreateWindowSizeDependentResources(unsigned, unsigned, const IRenderPassResourceCollection* = nullptr) override {}   // shadow maps do not follow the window
    void OnDestroyWindowSizeDependentResources() override {}
    bool Reserve(uint64_t InstancedTriangles) { return mWork.Reserve(vqhip_shadow_depth_work_bytes(InstancedTriangles, VQHIP_SHADOW_MAX_VIEWS)); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || p->NumSpotShadowViews > VQ_NUM_SHADOWING_LIGHTS__SPOT || p->NumPointShadowViews > VQ_NUM_SHADOWING_LIGHTS__POINT) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        vqhip_shadow_view views[kMaxViews];
        uint64_t triangles = 0;
        const int n = WalkViews(*p, views, [&](vqhip_shadow_view& v, const std::vector<vqhip_shadow_draw>& draws, ViewKind, unsigned) {
            v.draws = draws.data();
            for (const vqhip_shadow_draw& d : draws) triangles += InstancedTriangles(d);
        });
        mNumViews = n;
        if (n == 0) { mStatus = VQHIP_OK; return; }                              // nothing casts a shadow this frame
        if (!Reserve(triangles)) { mStatus = VQHIP_ERR_HIP; return; }
        mStatus = vqhip_shadow_depth(mCtx, p->Stream, views, n, mWork.ptr, mWork.bytes);
    }
    // The frame's views in the library's order — directional, spots, point faces (LINEAR_DEPTH, the caster's position and range) — into views[0 .. n): a view
    // whose draw list is missing or empty is skipped, a map array that is NULL stays NULL. perView(view, its draws, kind, k) sets view.draws; k is the spot's
    // number, or light * 6 + face. Returns n. Shared with MaskedShadowDepthPass (VIEW = vqhip_shadow_masked_view).
    static constexpr int kMaxViews = 1 + VQ_NUM_SHADOWING_LIGHTS__SPOT + 6 * VQ_NUM_SHADOWING_LIGHTS__POINT;
    enum ViewKind { kDirectional, kSpot, kPointFace };
    template <class VIEW, class FN>
    static int WalkViews(const FDrawParameters& p, VIEW* views, FN&& perView) {
        int n = 0;
        auto add = [&](const std::vector<vqhip_shadow_draw>* draws, ViewKind kind, unsigned k, float* maps, int dim, VQ_float3 pos, float farPlane) {
            if (!draws || draws->empty()) return;
            VIEW& v = views[n++];
            v.depth = maps ? maps + (size_t)k * dim * dim : nullptr; v.pitchBytes = 0; v.dim = dim; v.linearDepth = kind == kPointFace; v.cameraPosition = pos; v.farPlane = farPlane;
            v.draws = nullptr; v.numDraws = (int32_t)draws->size();
            perView(v, *draws, kind, k);
        };
        const VQ_float3 zero = { 0.0f, 0.0f, 0.0f };
        add(p.DirectionalDraws, kDirectional, 0, p.ShadowMapsDirectional, p.DirectionalDim, zero, 1.0f);            // :1146-1147
        for (unsigned i = 0; i < p.NumSpotShadowViews; ++i) add(p.SpotDraws[i], kSpot, i, p.ShadowMapsSpot, p.SpotDim, zero, 1.0f);
        for (unsigned i = 0; i < p.NumPointShadowViews * 6; ++i) add(p.PointDraws[i], kPointFace, i, p.ShadowMapsPoint, p.PointDim, p.PointPosition[i / 6], p.PointRange[i / 6]);
        return n;
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }
    size_t GetWorkBytes() const { return mWork.bytes; }
    int LastViewCount() const { return mNumViews; }
private:
    WorkBuffer mWork;
    int mNumViews = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Z pre-pass, depth half == VQRenderer::RenderDepthPrePass (SceneRendering.cpp:1265-1363) through FDepthPrePassPSOs: vqhip_scene_depth. FDrawParameters carries
// what the function holds: the main view's draw list (FSceneDrawData::mainViewDrawParams, each FInstancedDrawParameters as a vqhip_scene_depth_draw whose matrices
// are the uploaded PerObjectData), the stream and the depth target (DSV_SceneDepthMSAA when bMSAA, else DSV_SceneDepth, as R32F memory). W and H are the window's
// (OnCreateWindowSizeDependentResources, the viewport of :1330); bMSAA selects 4 samples, the engine's default, else 1. The primitive and layer planes are the
// library's addition (the masks vqhip_forward_lighting_msaa and vqhip_msaa_resolve_surfaces read); leave them NULL for the engine's own outputs. The pass's
// normals target stays with vqhip_scene_normals_from_materials; the interpolant planes are SceneInterpolantsPass's (below). The pass owns the work buffer, as
// ShadowDepthPass does.
// ---------------------------------------------------------------------------------------------------------------
class DepthPrePass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const std::vector<vqhip_scene_depth_draw>* Draws = nullptr;             // nullptr or empty: the target is cleared (:1318 clears before the draw loop)
        bool bMSAA = true;                                                      // SceneView.sceneParameters.bMSAA (:1268)
        float* SceneDepth = nullptr;                                            // [H][W] or, bMSAA, [H][W][4]
        uint32_t* Primitive = nullptr;                                          // optional, the shape of SceneDepth
        int NumLayers = 0;                                                      // bMSAA only
        uint8_t* Coverage[VQHIP_SCENE_DEPTH_MAX_LAYERS] = {};
        uint32_t* LayerPrimitive[VQHIP_SCENE_DEPTH_MAX_LAYERS] = {};
    };
    explicit DepthPrePass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { mWork.Release(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override { mWidth = Width; mHeight = Height; }
    void OnDestroyWindowSizeDependentResources() override { mWidth = mHeight = 0; }
    bool Reserve(uint64_t InstancedTriangles) { return mWork.Reserve(vqhip_scene_depth_work_bytes(InstancedTriangles)); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || p->NumLayers < 0 || p->NumLayers > VQHIP_SCENE_DEPTH_MAX_LAYERS) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        uint64_t triangles = 0;
        const int numDraws = p->Draws ? (int)p->Draws->size() : 0;
        for (int d = 0; d < numDraws; ++d) triangles += InstancedTriangles((*p->Draws)[d]);
        if (!Reserve(triangles)) { mStatus = VQHIP_ERR_HIP; return; }
        const vqhip_scene_depth_targets t = Targets(*p);
        mStatus = vqhip_scene_depth(mCtx, p->Stream, numDraws ? p->Draws->data() : nullptr, numDraws, (int)mWidth, (int)mHeight, p->bMSAA ? 4 : 1, &t, mWork.ptr, mWork.bytes);
    }
    static vqhip_scene_depth_targets Targets(const FDrawParameters& p) {        // shared with MaskedDepthPrePass; the layer planes exist with MSAA only
        vqhip_scene_depth_targets t = {};
        t.depth = p.SceneDepth; t.primitive = p.Primitive; t.layers = p.bMSAA ? p.NumLayers : 0;
        for (int k = 0; k < t.layers; ++k) { t.coverage[k] = p.Coverage[k]; t.layerPrimitive[k] = p.LayerPrimitive[k]; }
        return t;
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }
    size_t GetWorkBytes() const { return mWork.bytes; }
private:
    WorkBuffer mWork;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Z pre-pass with its "_AlphaMasked" draws == RenderDepthPrePass as the engine runs it on its default content (SceneRendering.cpp:1318-1337: the masked PSO and the
// diffuse SRV for materials with IsAlphaMasked): vqhip_scene_masked_depth (docs/DESIGN_DETAILS.md §7.19). FDrawParameters is DepthPrePass's plus what the
// function reads of the materials: MaterialIndex[d] names draw d's entry of Materials (the host array the *_from_materials calls take), a negative index or a
// missing list draws opaque. The pass builds the vqhip_scene_masked_depth_draw list — material = &Materials[index] — and counts the masked instanced triangles by
// the header's rule (texDiffuse.reserved has VQHIP_MATERIAL_ALPHA_MASKED) for the work size. A frame without a masked material enqueues what DepthPrePass enqueues.
// ---------------------------------------------------------------------------------------------------------------
class MaskedDepthPrePass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public DepthPrePass::FDrawParameters {
        const std::vector<int32_t>* MaterialIndex = nullptr;                    // per draw, the size of *Draws; < 0: no material (opaque)
        const vqhip_material* Materials = nullptr; int NumMaterials = 0;        // HOST
    };
    explicit MaskedDepthPrePass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { mWork.Release(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override { mWidth = Width; mHeight = Height; }
    void OnDestroyWindowSizeDependentResources() override { mWidth = mHeight = 0; }
    bool Reserve(uint64_t InstancedTriangles, uint64_t MaskedInstancedTriangles, int NumDraws) { return mWork.Reserve(vqhip_scene_masked_depth_work_bytes(InstancedTriangles, MaskedInstancedTriangles, NumDraws)); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || p->NumLayers < 0 || p->NumLayers > VQHIP_SCENE_DEPTH_MAX_LAYERS) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        const int numDraws = p->Draws ? (int)p->Draws->size() : 0;
        if (p->MaterialIndex && (int)p->MaterialIndex->size() != numDraws) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mDraws.resize((size_t)numDraws);
        uint64_t triangles = 0, masked = 0;
        for (int d = 0; d < numDraws; ++d) {
            vqhip_scene_masked_depth_draw& m = mDraws[(size_t)d];
            m.draw = (*p->Draws)[(size_t)d];
            const int32_t index = p->MaterialIndex ? (*p->MaterialIndex)[(size_t)d] : -1;
            if (index >= p->NumMaterials || (index >= 0 && !p->Materials)) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
            m.material = index >= 0 ? p->Materials + index : nullptr;
            const uint64_t n = InstancedTriangles(m.draw);
            triangles += n;
            if (m.material && (m.material->texDiffuse.reserved & VQHIP_MATERIAL_ALPHA_MASKED)) masked += n;
        }
        mMaskedTriangles = masked;
        if (!Reserve(triangles, masked, numDraws)) { mStatus = VQHIP_ERR_HIP; return; }
        const vqhip_scene_depth_targets t = DepthPrePass::Targets(*p);
        mStatus = vqhip_scene_masked_depth(mCtx, p->Stream, numDraws ? mDraws.data() : nullptr, numDraws, (int)mWidth, (int)mHeight, p->bMSAA ? 4 : 1, &t, mWork.ptr, mWork.bytes);
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }
    size_t GetWorkBytes() const { return mWork.bytes; }
    uint64_t LastMaskedTriangles() const { return mMaskedTriangles; }
private:
    WorkBuffer mWork;
    unsigned mWidth = 0, mHeight = 0;
    uint64_t mMaskedTriangles = 0;
    std::vector<vqhip_scene_masked_depth_draw> mDraws;                          // consumed by the call before it returns; kept to spare the allocation
};

// ---------------------------------------------------------------------------------------------------------------
// Shadow maps with their "_AlphaMasked" draws == DrawShadowViewMeshList picking the masked shadow PSO and binding the diffuse SRV for materials with
// IsAlphaMasked (SceneRendering.cpp:1008-1030): vqhip_shadow_masked_depth (§7.19). FDrawParameters is ShadowDepthPass's plus, per view, the material index of each
// draw (a list parallel to the view's draw list; a missing list or a negative index draws opaque) and the host material array. A draw is masked when its material's
// texDiffuse.reserved has VQHIP_MATERIAL_ALPHA_MASKED: texDiffuseAlpha = &material.texDiffuse — whose texels may be NULL: that shader has no HasDiffuseMap test, the
// draw then loses every fragment. Views with an empty draw list are skipped, as in ShadowDepthPass.
// ---------------------------------------------------------------------------------------------------------------
class MaskedShadowDepthPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public ShadowDepthPass::FDrawParameters {
        const std::vector<int32_t>* DirectionalMaterialIndex = nullptr;
        const std::vector<int32_t>* SpotMaterialIndex[VQ_NUM_SHADOWING_LIGHTS__SPOT] = {};
        const std::vector<int32_t>* PointMaterialIndex[VQ_NUM_SHADOWING_LIGHTS__POINT * 6] = {};
        const vqhip_material* Materials = nullptr; int NumMaterials = 0;        // HOST
    };
    explicit MaskedShadowDepthPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { mWork.Release(); }
    void OnCreateWindowSizeDependentResources(unsigned, unsigned, const IRenderPassResourceCollection* = nullptr) override {}   // shadow maps do not follow the window
    void OnDestroyWindowSizeDependentResources() override {}
    bool Reserve(uint64_t InstancedTriangles, uint64_t MaskedInstancedTriangles, int NumDraws) { return mWork.Reserve(vqhip_shadow_masked_depth_work_bytes(InstancedTriangles, MaskedInstancedTriangles, VQHIP_SHADOW_MAX_VIEWS, NumDraws)); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || p->NumSpotShadowViews > VQ_NUM_SHADOWING_LIGHTS__SPOT || p->NumPointShadowViews > VQ_NUM_SHADOWING_LIGHTS__POINT) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        vqhip_shadow_masked_view views[ShadowDepthPass::kMaxViews];
        size_t first[ShadowDepthPass::kMaxViews];                                // where each view's draws start in mDraws (the vector may move while it grows)
        uint64_t triangles = 0, masked = 0;
        bool ok = true;
        mDraws.clear();
        const int n = ShadowDepthPass::WalkViews(*p, views, [&](vqhip_shadow_masked_view& v, const std::vector<vqhip_shadow_draw>& draws, ShadowDepthPass::ViewKind kind, unsigned slot) {
            const std::vector<int32_t>* index = kind == ShadowDepthPass::kDirectional ? p->DirectionalMaterialIndex : kind == ShadowDepthPass::kSpot ? p->SpotMaterialIndex[slot] : p->PointMaterialIndex[slot];
            if (index && index->size() != draws.size()) { ok = false; return; }
            first[&v - views] = mDraws.size();
            for (size_t d = 0; d < draws.size(); ++d) {
                vqhip_shadow_masked_draw m;
                m.draw = draws[d];
                m.texDiffuseAlpha = nullptr;
                const int32_t k = index ? (*index)[d] : -1;
                if (k >= p->NumMaterials || (k >= 0 && !p->Materials)) { ok = false; return; }
                const uint64_t t = InstancedTriangles(m.draw);
                triangles += t;
                if (k >= 0 && (p->Materials[k].texDiffuse.reserved & VQHIP_MATERIAL_ALPHA_MASKED)) { m.texDiffuseAlpha = &p->Materials[k].texDiffuse; masked += t; }
                mDraws.push_back(m);
            }
        });
        if (!ok) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mNumViews = n; mMaskedTriangles = masked;
        if (n == 0) { mStatus = VQHIP_OK; return; }                              // nothing casts a shadow this frame
        for (int v = 0; v < n; ++v) views[v].draws = mDraws.data() + first[v];
        if (!Reserve(triangles, masked, (int)mDraws.size())) { mStatus = VQHIP_ERR_HIP; return; }
        mStatus = vqhip_shadow_masked_depth(mCtx, p->Stream, views, n, mWork.ptr, mWork.bytes);
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }
    size_t GetWorkBytes() const { return mWork.bytes; }
    int LastViewCount() const { return mNumViews; }
    uint64_t LastMaskedTriangles() const { return mMaskedTriangles; }
private:
    WorkBuffer mWork;
    int mNumViews = 0;
    uint64_t mMaskedTriangles = 0;
    std::vector<vqhip_shadow_masked_draw> mDraws;                               // all views' draws, consumed by the call before it returns
};

// ---------------------------------------------------------------------------------------------------------------
// The lit draw's vertex stage and interpolation == what VQRenderer::RenderSceneColor (SceneRendering.cpp:1619-1760) leaves to the rasteriser between the draw call
// and PSMain: vqhip_scene_interpolants. FDrawParameters carries the pass's draw list (FSceneDrawData::mainViewDrawParams again, each FInstancedDrawParameters as a
// vqhip_scene_surface_draw whose four matrix blocks are the uploaded PerObjectLightingData and whose materialIndex is the draw's material) — the SAME list, in the
// same order, that DepthPrePass rasterised — and the owner plane DepthPrePass wrote: Primitive without MSAA, one LayerPrimitive[k] per call with it. The planes
// written are HipSceneColorPass's pInterpolants (and its svPosition planes when SvPositionCurr / SvPositionPrev are given). W and H are the window's. The pass owns
// the work buffer (the draw table's device home).
// ---------------------------------------------------------------------------------------------------------------
class SceneInterpolantsPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const std::vector<vqhip_scene_surface_draw>* Draws = nullptr;           // nullptr or empty: every pixel receives the no-owner record
        const uint32_t* Owner = nullptr;                                        // [H][OwnerPitch]
        int OwnerPitch = 0;                                                     // pixels per row, 0 = W
        void* Ip0 = nullptr; void* Ip1 = nullptr; void* Ip2 = nullptr;          // float4 [H][W]
        void* SvPositionCurr = nullptr; void* SvPositionPrev = nullptr;         // both or neither
    };
    explicit SceneInterpolantsPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { mWork.Release(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override { mWidth = Width; mHeight = Height; }
    void OnDestroyWindowSizeDependentResources() override { mWidth = mHeight = 0; }
    bool Reserve(int NumDraws) { return mWork.Reserve(vqhip_scene_interpolants_work_bytes(NumDraws)); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        const int numDraws = p->Draws ? (int)p->Draws->size() : 0;
        if (!Reserve(numDraws)) { mStatus = VQHIP_ERR_HIP; return; }
        vqhip_scene_interpolant_targets t = {};
        t.ip0 = p->Ip0; t.ip1 = p->Ip1; t.ip2 = p->Ip2; t.svPositionCurr = p->SvPositionCurr; t.svPositionPrev = p->SvPositionPrev;
        mStatus = vqhip_scene_interpolants(mCtx, p->Stream, numDraws ? p->Draws->data() : nullptr, numDraws, (int)mWidth, (int)mHeight, p->Owner, p->OwnerPitch, &t,
                                           mWork.ptr, mWork.bytes);
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }
    size_t GetWorkBytes() const { return mWork.bytes; }
private:
    WorkBuffer mWork;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// The same resolve with the helper lanes' uv (docs/DESIGN_DETAILS.md §7.20): vqhip_scene_quad_interpolants. The inputs are SceneInterpolantsPass's; QuadUV is one
// more float4 plane of the window's size, which QuadLitDrawPass below reads so that Texture2D.Sample takes the derivatives D3D's helper lanes give — the ones
// MaskedDepthPrePass already used for its discard. The pass owns the work buffer and remembers the plane of its last successful call.
// ---------------------------------------------------------------------------------------------------------------
class QuadInterpolantsPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public SceneInterpolantsPass::FDrawParameters {
        void* QuadUV = nullptr;                                                 // float4 [H][QuadPitch], required
        int QuadPitch = 0;                                                      // pixels per row, 0 = W
    };
    explicit QuadInterpolantsPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { mWork.Release(); mQuadUV = nullptr; mQuadPitch = 0; }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override { mWidth = Width; mHeight = Height; }
    void OnDestroyWindowSizeDependentResources() override { mWidth = mHeight = 0; mQuadUV = nullptr; mQuadPitch = 0; }
    bool Reserve(int NumDraws) { return mWork.Reserve(vqhip_scene_interpolants_work_bytes(NumDraws)); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        mQuadUV = nullptr; mQuadPitch = 0;
        if (!p) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        const int numDraws = p->Draws ? (int)p->Draws->size() : 0;
        if (!Reserve(numDraws)) { mStatus = VQHIP_ERR_HIP; return; }
        vqhip_scene_quad_targets t = {};
        t.planes.ip0 = p->Ip0; t.planes.ip1 = p->Ip1; t.planes.ip2 = p->Ip2; t.planes.svPositionCurr = p->SvPositionCurr; t.planes.svPositionPrev = p->SvPositionPrev;
        t.quadUV = p->QuadUV; t.quad_pitch = p->QuadPitch;
        mStatus = vqhip_scene_quad_interpolants(mCtx, p->Stream, numDraws ? p->Draws->data() : nullptr, numDraws, (int)mWidth, (int)mHeight, p->Owner, p->OwnerPitch, &t,
                                                mWork.ptr, mWork.bytes);
        if (mStatus == VQHIP_OK) { mQuadUV = p->QuadUV; mQuadPitch = p->QuadPitch ? p->QuadPitch : (int)mWidth; }
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }
    size_t GetWorkBytes() const { return mWork.bytes; }
    const void* GetQuadUV() const { return mQuadUV; }            // nullptr until a call succeeded
    int GetQuadPitch() const { return mQuadPitch; }              // pixels per row
private:
    WorkBuffer mWork;
    const void* mQuadUV = nullptr; int mQuadPitch = 0;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// The lit draw over planes QuadInterpolantsPass wrote == PSMain with D3D's helper-lane derivatives (§7.20 Q2). One parameter block, three uses, each a _quad
// producer: pGBufferOut given -> vqhip_gbuffer_from_materials_quad into the caller's planes (one 4x layer; vqhip_forward_lighting_msaa shades them);
// pSceneNormalsOut given -> vqhip_scene_normals_from_materials_quad (the Z pre-pass's colour target); neither -> vqhip_forward_lighting_from_materials_quad
// into the pass's own scene colour (RGBA16F), with the draw's other render targets when asked for. The quad-uv plane is taken from the resolve pass.
// ---------------------------------------------------------------------------------------------------------------
class QuadLitDrawPass : public RenderPassBase {
public:
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const QuadInterpolantsPass* pQuadInterpolants = nullptr;  // the resolve whose last call wrote *pInterpolants and the quad-uv plane
        const vqhip_interpolants* pInterpolants = nullptr;
        const vqhip_material* pMaterials = nullptr;
        int NumMaterials = 0;
        const vqhip_ssao* pScreenSpaceAO = nullptr;
        const VQ_PerFrameData* pPerFrame = nullptr;
        const VQ_PerViewLightingData* pPerView = nullptr;
        const VQ_PointLight* pExtraPointLights = nullptr;
        int NumExtraPointLights = 0;
        const vqhip_envmap* pEnvironmentMap = nullptr;
        const vqhip_shadowmaps* pShadowMaps = nullptr;
        const vqhip_psmain_targets* pTargets = nullptr;          // the fused draw's other render targets, or nullptr
        const vqhip_gbuffer* pGBufferOut = nullptr;              // one 4x layer's record planes instead of the lit frame
        void* pSceneNormalsOut = nullptr;                        // Tex_SceneNormals (R10G10B10A2_UNORM, tightly packed) instead of the lit frame
    };
    explicit QuadLitDrawPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~QuadLitDrawPass() override { Free(mSceneColor); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { OnDestroyWindowSizeDependentResources(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override {
        Free(mSceneColor);
        mWidth = Width; mHeight = Height;
        mSceneColor = Alloc((size_t)Width * Height * 8);
    }
    void OnDestroyWindowSizeDependentResources() override { Free(mSceneColor); mWidth = mHeight = 0; }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !p->pInterpolants || !p->pQuadInterpolants || !p->pQuadInterpolants->GetQuadUV() || (p->pGBufferOut && p->pSceneNormalsOut)) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        const void* quadUV = p->pQuadInterpolants->GetQuadUV();
        const int quadPitch = p->pQuadInterpolants->GetQuadPitch();
        if (p->pSceneNormalsOut) {
            mStatus = vqhip_scene_normals_from_materials_quad(mCtx, p->Stream, p->pInterpolants, p->pMaterials, p->NumMaterials, p->pSceneNormalsOut,
                                                              VQHIP_FMT_R10G10B10A2_UNORM, 0, quadUV, quadPitch);
            return;
        }
        if (!p->pPerFrame) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        if (p->pGBufferOut) {
            mStatus = vqhip_gbuffer_from_materials_quad(mCtx, p->Stream, p->pInterpolants, p->pMaterials, p->NumMaterials, p->pPerFrame->fAmbientLightingFactor,
                                                        p->pScreenSpaceAO, p->pGBufferOut, quadUV, quadPitch);
            return;
        }
        if (!mSceneColor) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mStatus = vqhip_forward_lighting_from_materials_quad(mCtx, p->Stream, p->pInterpolants, p->pMaterials, p->NumMaterials, p->pScreenSpaceAO, p->pPerFrame, p->pPerView,
                                                             p->pExtraPointLights, p->NumExtraPointLights, p->pEnvironmentMap, p->pShadowMaps, mSceneColor, (int)mWidth,
                                                             VQHIP_FMT_RGBA16F, p->pTargets, quadUV, quadPitch);
    }
    void* GetSceneColor() const { return mSceneColor; }          // RGBA16F, width * height
private:
    void* mSceneColor = nullptr;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Reflection denoiser, pass 1 == the "FFX DNSR Reproject" dispatch of ScreenSpaceReflectionsPass::RecordCommands: vqhip_ssr_reproject. Buffer roles as
// ScreenSpaceReflections.cpp:1177-1198 binds them for frame index i: reads the surfaces of this frame and their history copies, TexRadiance[i] (what the march
// wrote), TexRadiance[1 - i] (last frame's resolved radiance), the motion vectors, TexVariance[1 - i] and TexSampleCount[1 - i]; writes TexReprojectedRadiance,
// TexAvgRadiance[i], TexVariance[i], TexSampleCount[i]. TexAvgRadiance[1 - i] and the blue noise are bound by the engine and never read by the shader: not
// parameters. The pass owns nothing, the caller ping-pongs; the engine's bClearHistoryBuffers is a plain clear of the history planes by the caller.
// ---------------------------------------------------------------------------------------------------------------
class HipSSRReprojectPass : public OwnsNothingPass {
public:
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        VQ_SSSRConstants ffxCBuffer = {};
        const uint32_t* TexDenoiserTileList = nullptr;           // HipSSRIntersectPass::GetDenoiserTileList()
        const uint32_t* TexRayCounter = nullptr;                 // HipSSRIntersectPass::GetRayCounter(): [1] = tiles
        const float* TexDepthHierarchy = nullptr;                // mip 0, R32F
        const uint8_t* TexExtractedRoughness = nullptr;          // R8_UNORM
        const void* TexNormals = nullptr;                        // R10G10B10A2_UNORM
        const float* TexDepthHistory = nullptr;                  // R32F
        const uint8_t* TexRoughnessHistory = nullptr;            // R8_UNORM
        const void* TexNormalsHistory = nullptr;                 // R10G10B10A2_UNORM
        const void* TexRadianceIn = nullptr;                     // TexRadiance[i], RGBA16F (alpha = ray length)
        const void* TexRadianceHistory = nullptr;                // TexRadiance[1 - i], RGBA16F
        const void* TexMotionVectors = nullptr;                  // Tex_SceneMotionVectors, RG16F
        const void* TexVarianceHistory = nullptr;                // TexVariance[1 - i], R16F
        const void* TexSampleCountHistory = nullptr;             // TexSampleCount[1 - i], R16F
        void* TexReprojectedRadiance = nullptr;                  // RGBA16F
        void* TexAvgRadianceOut = nullptr;                       // TexAvgRadiance[i], R11G11B10_FLOAT, ceil(w/8) x ceil(h/8)
        void* TexVarianceOut = nullptr;                          // TexVariance[i], R16F
        void* TexSampleCountOut = nullptr;                       // TexSampleCount[i], R16F
    };
    explicit HipSSRReprojectPass(vqhip_ctx* Ctx) : OwnsNothingPass(Ctx) {}
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        vqhip_ssr_reproject_surfaces s = {};
        s.tile_list = p->TexDenoiserTileList; s.counters = p->TexRayCounter;
        s.depth = p->TexDepthHierarchy; s.normals = p->TexNormals; s.roughness = p->TexExtractedRoughness;
        s.depth_history = p->TexDepthHistory; s.normal_history = p->TexNormalsHistory; s.roughness_history = p->TexRoughnessHistory;
        s.radiance = p->TexRadianceIn; s.radiance_history = p->TexRadianceHistory; s.motion_vectors = p->TexMotionVectors;
        s.variance_history = p->TexVarianceHistory; s.sample_count_history = p->TexSampleCountHistory;
        s.out_reprojected = p->TexReprojectedRadiance; s.out_average = p->TexAvgRadianceOut; s.out_variance = p->TexVarianceOut; s.out_sample_count = p->TexSampleCountOut;
        s.normals_fmt = s.normal_history_fmt = VQHIP_FMT_R10G10B10A2_UNORM;
        s.radiance_fmt = s.radiance_history_fmt = s.out_reprojected_fmt = VQHIP_FMT_RGBA16F;
        s.motion_fmt = VQHIP_FMT_RG16F; s.out_average_fmt = VQHIP_FMT_R11G11B10_FLOAT;
        mStatus = vqhip_ssr_reproject(mCtx, p->Stream, &s, &p->ffxCBuffer);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// Reflection denoiser, pass 2 == the "FFX DNSR Prefilter" dispatch of ScreenSpaceReflectionsPass::RecordCommands (ScreenSpaceReflections.cpp:387-397):
// vqhip_ssr_prefilter. Reads TexRadiance[i] / TexVariance[i] / TexAvgRadiance[i] and writes TexRadiance[1 - i] / TexVariance[1 - i] (:1199-1212): the pass owns
// nothing, the caller ping-pongs. Pixels of unlisted tiles are not written.
// ---------------------------------------------------------------------------------------------------------------
class HipSSRPrefilterPass : public OwnsNothingPass {
public:
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        VQ_SSSRConstants ffxCBuffer = {};
        const uint32_t* TexDenoiserTileList = nullptr;           // HipSSRIntersectPass::GetDenoiserTileList()
        const uint32_t* TexRayCounter = nullptr;                 // HipSSRIntersectPass::GetRayCounter(): [1] = tiles
        const float* TexDepthHierarchy = nullptr;                // mip 0, R32F
        const void* TexNormals = nullptr;                        // R10G10B10A2_UNORM
        const uint8_t* TexExtractedRoughness = nullptr;          // R8_UNORM
        const void* TexAvgRadiance = nullptr;                    // R11G11B10_FLOAT, ceil(w/8) x ceil(h/8)
        const void* TexRadianceIn = nullptr;                     // TexRadiance[i], RGBA16F
        const void* TexVarianceIn = nullptr;                     // TexVariance[i], R16F
        void* TexRadianceOut = nullptr;                          // TexRadiance[1 - i]
        void* TexVarianceOut = nullptr;                          // TexVariance[1 - i]
    };
    explicit HipSSRPrefilterPass(vqhip_ctx* Ctx) : OwnsNothingPass(Ctx) {}
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mStatus = vqhip_ssr_prefilter(mCtx, p->Stream, p->TexDenoiserTileList, p->TexRayCounter, p->TexDepthHierarchy, 0, p->TexNormals, VQHIP_FMT_R10G10B10A2_UNORM, 0,
                                      p->TexExtractedRoughness, p->TexAvgRadiance, VQHIP_FMT_R11G11B10_FLOAT, p->TexRadianceIn, VQHIP_FMT_RGBA16F, 0, p->TexVarianceIn, 0,
                                      &p->ffxCBuffer, p->TexRadianceOut, VQHIP_FMT_RGBA16F, 0, p->TexVarianceOut, 0);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// Reflection denoiser, pass 3 == the "FFX DNSR Resolve Temporal" dispatch (ScreenSpaceReflections.cpp:413-423): vqhip_ssr_resolve_temporal. Reads what the
// prefilter wrote (TexRadiance[1 - i], TexVariance[1 - i]), TexReprojectedRadiance and TexSampleCount[1 - i] (:1214-1222), writes TexRadiance[i] / TexVariance[i] —
// the image vqhip_composite_reflections consumes (:1230).
// ---------------------------------------------------------------------------------------------------------------
class HipSSRResolveTemporalPass : public OwnsNothingPass {
public:
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        VQ_SSSRConstants ffxCBuffer = {};
        const uint32_t* TexDenoiserTileList = nullptr;
        const uint32_t* TexRayCounter = nullptr;
        const uint8_t* TexExtractedRoughness = nullptr;
        const void* TexAvgRadiance = nullptr;                    // R11G11B10_FLOAT
        const void* TexRadianceIn = nullptr;                     // TexRadiance[1 - i], RGBA16F (the prefiltered radiance)
        const void* TexReprojectedRadiance = nullptr;            // RGBA16F
        const void* TexVarianceIn = nullptr;                     // TexVariance[1 - i], R16F
        const void* TexSampleCountIn = nullptr;                  // TexSampleCount[1 - i], R16F
        void* TexRadianceOut = nullptr;                          // TexRadiance[i]
        void* TexVarianceOut = nullptr;                          // TexVariance[i]
    };
    explicit HipSSRResolveTemporalPass(vqhip_ctx* Ctx) : OwnsNothingPass(Ctx) {}
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mStatus = vqhip_ssr_resolve_temporal(mCtx, p->Stream, p->TexDenoiserTileList, p->TexRayCounter, p->TexExtractedRoughness, p->TexAvgRadiance, VQHIP_FMT_R11G11B10_FLOAT,
                                             p->TexRadianceIn, VQHIP_FMT_RGBA16F, 0, p->TexReprojectedRadiance, VQHIP_FMT_RGBA16F, 0, p->TexVarianceIn, 0, p->TexSampleCountIn, 0,
                                             &p->ffxCBuffer, p->TexRadianceOut, VQHIP_FMT_RGBA16F, 0, p->TexVarianceOut, 0);
    }
};

// ---------------------------------------------------------------------------------------------------------------
// Z pre-pass colour target == the pixel-shader half of VQRenderer::RenderDepthPrePass (SceneRendering.cpp:1264-1360, DepthPrePass.hlsl:PSMain): owns
// Tex_SceneNormals (R10G10B10A2_UNORM, RenderResources.cpp:185-197) — HipSSREnvironmentFallbackPass::FDrawParameters::TexNormals. The depth target of the
// same draws is DepthPrePass's (above); the interpolant planes are SceneInterpolantsPass's.
// ---------------------------------------------------------------------------------------------------------------
class HipDepthPrePassNormals : public RenderPassBase {
public:
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const vqhip_interpolants* pInterpolants = nullptr;       // the rasterised PSInput (DepthPrePass.hlsl:38-49: the same five attributes the lit draws get)
        const vqhip_material* pMaterials = nullptr;              // cbPerObject.materialData + texDiffuse / texNormals of every material on screen
        int NumMaterials = 0;
    };
    explicit HipDepthPrePassNormals(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~HipDepthPrePassNormals() override { OnDestroyWindowSizeDependentResources(); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { OnDestroyWindowSizeDependentResources(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override {
        OnDestroyWindowSizeDependentResources();
        mWidth = Width; mHeight = Height;
        mSceneNormals = Alloc((size_t)Width * Height * 4);
    }
    void OnDestroyWindowSizeDependentResources() override { Free(mSceneNormals); mWidth = mHeight = 0; }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !mSceneNormals) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mStatus = vqhip_scene_normals_from_materials(mCtx, p->Stream, p->pInterpolants, p->pMaterials, p->NumMaterials, mSceneNormals, VQHIP_FMT_R10G10B10A2_UNORM, (int)mWidth);
    }
    void* GetSceneNormals() const { return mSceneNormals; }      // R10G10B10A2_UNORM, width*height uint32
private:
    void* mSceneNormals = nullptr;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Picking == ObjectIDPass::RecordCommands (ObjectIDPass.cpp:160-278) and its ReadBackPixel (:283-303): the pass's OWN depth call — the main view's draw list
// through vqhip_scene_masked_depth at one sample with EVERY draw's cullMode forced to VQHIP_CULL_NONE (the pass ignores iFaceCull; a frame without a masked material
// enqueues what vqhip_scene_depth enqueues) — and then vqhip_object_ids over that call's owner plane (docs/DESIGN_DETAILS.md §7.21 P0). FDrawParameters is
// MaskedDepthPrePass's draw list and materials plus, per draw, what ObjectID.hlsl writes: the uploaded ObjID block, the mesh id and the material id. The pass owns
// its depth plane (the pass's D32), the owner plane, the ids plane (the pass's R32G32B32A32_SINT target) and both work buffers. W and H are the window's.
// ---------------------------------------------------------------------------------------------------------------
class ObjectIDPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FObjectID { const int32_t* ObjID = nullptr; int32_t MeshID = 0; int32_t MaterialID = 0; };   // ObjID: device, int4 [numInstances]
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const std::vector<vqhip_scene_depth_draw>* Draws = nullptr;             // the main view's draw list; cullMode is ignored. nullptr or empty: ids all zero
        const std::vector<FObjectID>* IDs = nullptr;                            // per draw, the size of *Draws
        const std::vector<int32_t>* MaterialIndex = nullptr;                    // per draw, or nullptr; < 0: no material (opaque) — as MaskedDepthPrePass
        const vqhip_material* Materials = nullptr; int NumMaterials = 0;        // HOST
    };
    explicit ObjectIDPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    ~ObjectIDPass() override { OnDestroyWindowSizeDependentResources(); }
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { OnDestroyWindowSizeDependentResources(); mDepthWork.Release(); mIdsWork.Release(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override {
        OnDestroyWindowSizeDependentResources();
        mWidth = Width; mHeight = Height;
        const size_t px = (size_t)Width * Height;
        mDepth = Alloc(px * 4); mOwner = Alloc(px * 4); mIds = Alloc(px * 16);
    }
    void OnDestroyWindowSizeDependentResources() override { Free(mDepth); Free(mOwner); Free(mIds); mWidth = mHeight = 0; }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !mDepth || !mOwner || !mIds) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        const int numDraws = p->Draws ? (int)p->Draws->size() : 0;
        if ((numDraws && (!p->IDs || (int)p->IDs->size() != numDraws)) || (p->MaterialIndex && (int)p->MaterialIndex->size() != numDraws)) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        mDraws.resize((size_t)numDraws); mIdDraws.resize((size_t)numDraws);
        uint64_t triangles = 0, masked = 0;
        for (int d = 0; d < numDraws; ++d) {
            vqhip_scene_masked_depth_draw& m = mDraws[(size_t)d];
            m.draw = (*p->Draws)[(size_t)d];
            m.draw.cullMode = VQHIP_CULL_NONE;                                   // ObjectIDPass.cpp: one rasteriser state for every draw
            const int32_t index = p->MaterialIndex ? (*p->MaterialIndex)[(size_t)d] : -1;
            if (index >= p->NumMaterials || (index >= 0 && !p->Materials)) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
            m.material = index >= 0 ? p->Materials + index : nullptr;
            const uint64_t n = InstancedTriangles(m.draw);
            triangles += n;
            if (m.material && (m.material->texDiffuse.reserved & VQHIP_MATERIAL_ALPHA_MASKED)) masked += n;
            const FObjectID& id = (*p->IDs)[(size_t)d];
            vqhip_object_id_draw& o = mIdDraws[(size_t)d];
            o.numIndices = m.draw.mesh.numIndices; o.numInstances = m.draw.numInstances; o.objID = id.ObjID; o.meshID = id.MeshID; o.materialID = id.MaterialID;
        }
        if (!mDepthWork.Reserve(vqhip_scene_masked_depth_work_bytes(triangles, masked, numDraws)) || !mIdsWork.Reserve(vqhip_object_ids_work_bytes(numDraws))) { mStatus = VQHIP_ERR_HIP; return; }
        vqhip_scene_depth_targets t = {};
        t.depth = (float*)mDepth; t.primitive = (uint32_t*)mOwner;
        mStatus = vqhip_scene_masked_depth(mCtx, p->Stream, numDraws ? mDraws.data() : nullptr, numDraws, (int)mWidth, (int)mHeight, 1, &t, mDepthWork.ptr, mDepthWork.bytes);
        if (mStatus != VQHIP_OK) return;
        mStatus = vqhip_object_ids(mCtx, p->Stream, numDraws ? mIdDraws.data() : nullptr, numDraws, (int)mWidth, (int)mHeight, (const uint32_t*)mOwner, 0, (int32_t*)mIds, 0,
                                   mIdsWork.ptr, mIdsWork.bytes);
    }
    // ObjectIDPass::ReadBackPixel: the int4 at (X, Y) of the ids plane after the work enqueued on Stream — one 16-byte copy and a stream wait. Coordinates outside
    // the window (and a failed copy) return (-1, -1, -1, -1), as the reference does.
    struct FPixel { int32_t x, y, z, w; };
    FPixel ReadBackPixel(int X, int Y, void* Stream = nullptr) const {
        FPixel px = { -1, -1, -1, -1 };
        if (!mIds || X < 0 || Y < 0 || X >= (int)mWidth || Y >= (int)mHeight) return px;
        FPixel got;
        const char* src = (const char*)mIds + ((size_t)Y * mWidth + (size_t)X) * 16;
        if (hipMemcpyAsync(&got, src, 16, hipMemcpyDeviceToHost, (hipStream_t)Stream) != hipSuccess || hipStreamSynchronize((hipStream_t)Stream) != hipSuccess) return px;
        return got;
    }
    const int32_t* GetObjectIDs() const { return (const int32_t*)mIds; }          // int4 [H][W]
    const float* GetDepth() const { return (const float*)mDepth; }                // the pass's own depth, [H][W]
    const uint32_t* GetOwner() const { return (const uint32_t*)mOwner; }          // [H][W]
    size_t GetDepthWorkBytes() const { return mDepthWork.bytes; }
    size_t GetIdsWorkBytes() const { return mIdsWork.bytes; }
private:
    WorkBuffer mDepthWork, mIdsWork;
    void* mDepth = nullptr; void* mOwner = nullptr; void* mIds = nullptr;
    unsigned mWidth = 0, mHeight = 0;
    std::vector<vqhip_scene_masked_depth_draw> mDraws;                          // consumed by the calls before they return; kept to spare the allocations
    std::vector<vqhip_object_id_draw> mIdDraws;
};

// ---------------------------------------------------------------------------------------------------------------
// Selection highlight == OutlinePass::RecordCommands (OutlinePass.cpp:247-405), drawn last into scene colour by VQRenderer::RenderOutline
// (SceneRendering.cpp:514): vqhip_outline, both passes in one call at one sample per pixel (docs/DESIGN_DETAILS.md §7.21 O1 .. O6). FDrawParameters carries the
// selected draws (FSceneDrawData::outlineRenderParams, each FOutlineRenderData as a vqhip_outline_draw whose cb is the uploaded OutlineData block) and the scene
// colour to write into (RGBA16F, HipSceneColorPass's). Selection and Writer are the library's additions (the stencil mark and the draw each written pixel took its
// colour from); leave them NULL for the engine's own output. W and H are the window's. The pass owns the work buffer. With MSAA the engine draws the outline
// into the multisampled target: that form is not built (§7.21), the call refuses nothing but writes the one-sample picture.
// ---------------------------------------------------------------------------------------------------------------
class OutlinePass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const std::vector<vqhip_outline_draw>* Draws = nullptr;                 // nullptr or empty: nothing selected — scene colour stays, Selection / Writer are cleared
        void* SceneColor = nullptr;                                             // RGBA16F [H][SceneColorPitch], modified in place
        int SceneColorPitch = 0;                                                // pixels per row, 0 = W
        uint8_t* Selection = nullptr;                                           // optional, [H][W]
        uint32_t* Writer = nullptr;                                             // optional, [H][W]
    };
    explicit OutlinePass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { mWork.Release(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override { mWidth = Width; mHeight = Height; }
    void OnDestroyWindowSizeDependentResources() override { mWidth = mHeight = 0; }
    bool Reserve(uint64_t Triangles) { return mWork.Reserve(vqhip_outline_work_bytes(Triangles)); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !p->SceneColor) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        uint64_t triangles = 0;
        const int numDraws = p->Draws ? (int)p->Draws->size() : 0;
        for (int d = 0; d < numDraws; ++d) triangles += (*p->Draws)[(size_t)d].mesh.numIndices / 3;
        if (!Reserve(triangles)) { mStatus = VQHIP_ERR_HIP; return; }
        vqhip_outline_targets t = {};
        t.sceneColor = p->SceneColor; t.pitch = p->SceneColorPitch; t.selection = p->Selection; t.writer = p->Writer;
        mStatus = vqhip_outline(mCtx, p->Stream, numDraws ? p->Draws->data() : nullptr, numDraws, (int)mWidth, (int)mHeight, &t, mWork.ptr, mWork.bytes);
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }
    size_t GetWorkBytes() const { return mWork.bytes; }
private:
    WorkBuffer mWork;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// Heightmap displacement == CalcHeightOffset of the five vertex stages (ForwardLighting.hlsl:136-154, DepthPrePass.hlsl:96-100, ShadowDepthPass.hlsl:61-66,
// ObjectID.hlsl:70-74, Outline.hlsl:78-82), run ONCE per (mesh LOD, material with a height map and displacement != 0) instead of in every pass, view and frame:
// vqhip_displace_meshes (docs/DESIGN_DETAILS.md §7.22 H1 .. H4). Not a pass of the reference's frame: a load-time step, called again only when a material's tiling
// or displacement changes. Each FMesh asks for the full-stride stream (the lit, Outline and masked draws), the 12-byte stream (the opaque depth and shadow draws)
// or both; the pass owns nothing — the caller brings the vertex buffers, the height map and the output streams, and afterwards points mesh.positions of every
// draw of that (mesh, material) pair at the stream of its kind. Host-only code: the job table is built here, everything else happens in the library.
// ---------------------------------------------------------------------------------------------------------------
class HeightmapDisplacementPass : public OwnsNothingPass {
public:
    struct FMesh {
        const void* Vertices = nullptr; uint32_t StrideBytes = 44; uint32_t NumVertices = 0;   // device: the mesh LOD's vertex buffer (the engine's vertex)
        vqhip_texture2d Heightmap = {};                                                        // the material's SRVHeightMap; texels NULL: the null SRV
        VQ_float4 uvScaleOffset = { 1.0f, 1.0f, 0.0f, 0.0f };                                  // MaterialData.uvScaleOffset (tiling, uv_bias)
        float Displacement = 0.0f;                                                             // MaterialData.displacement
        void* OutFull = nullptr;                                                               // device, NumVertices * StrideBytes bytes, or nullptr: not wanted
        void* OutPositions = nullptr;                                                          // device, NumVertices * 12 bytes, or nullptr: not wanted
    };
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const std::vector<FMesh>* Meshes = nullptr;                                            // nullptr or empty: nothing to do
    };
    explicit HeightmapDisplacementPass(vqhip_ctx* Ctx) : OwnsNothingPass(Ctx) {}
    // the jobs of a mesh list: one per stream asked for, in the order of the list (full before positions)
    static void BuildJobs(const std::vector<FMesh>& Meshes, std::vector<vqhip_displace_job>& Jobs) {
        Jobs.clear();
        for (const FMesh& m : Meshes) {
            vqhip_displace_job j = {};
            j.vertices = m.Vertices; j.strideBytes = m.StrideBytes; j.numVertices = m.NumVertices;
            j.heightmap = m.Heightmap; j.uvScaleOffset = m.uvScaleOffset; j.displacement = m.Displacement;
            if (m.OutFull) { j.out = m.OutFull; j.outStrideBytes = m.StrideBytes; Jobs.push_back(j); }
            if (m.OutPositions) { j.out = m.OutPositions; j.outStrideBytes = 12; Jobs.push_back(j); }
        }
    }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        if (p->Meshes) BuildJobs(*p->Meshes, mJobs); else mJobs.clear();
        mStatus = vqhip_displace_meshes(mCtx, p->Stream, mJobs.empty() ? nullptr : mJobs.data(), (int)mJobs.size());
    }
    size_t GetNumJobs() const { return mJobs.size(); }                                         // of the last RecordCommands
private:
    std::vector<vqhip_displace_job> mJobs;                                                     // consumed by the call before it returns; kept to spare the allocation
};

// ---------------------------------------------------------------------------------------------------------------
// The unlit draws of the lit pass == the "Lights" loop of VQRenderer::RenderSceneColor (SceneRendering.cpp:1787-1819, UNLIT_PSO) and the solid half of
// VQRenderer::RenderLightBounds (:1940-1989, UNLIT_PSO or UNLIT_BLEND_PSO): vqhip_unlit_draws at one sample per pixel (docs/DESIGN_DETAILS.md §7.23 U1 .. U7).
// Each FLightRenderData is a vqhip_unlit_draw whose cb is the uploaded FFrameConstantBufferUnlit block (the engine fills it as it does today: color, and
// matModelViewProj = matWorldTransformation * SceneView.viewProj) and whose cullMode is VQHIP_CULL_BACK. The two fronts fill the parameter block as the two call
// sites bind their pipeline state:
//   LightMeshes : opaque, into scene colour.
//   LightBounds : bReflectionsEnabled — opaque into the cleared Tex_SceneColorBoundingVolumes (the plane vqhip_composite_reflections blends, :2296-2336; the
//                 caller clears it, as the engine does); otherwise blended straight into scene colour (:507-510).
// Depth is the scene's (HipDepthPrePass's, one sample), tested LESS and never written. Writer is the library's addition; leave it NULL for the engine's own
// output. W and H are the window's. The pass owns the work buffer. The wireframe half of RenderLightBounds is WireframePass::LightBounds
// (below); the MSAA PSOs are not built (§7.23).
// ---------------------------------------------------------------------------------------------------------------
class UnlitDrawsPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const std::vector<vqhip_unlit_draw>* Draws = nullptr;                   // nullptr or empty: nothing to draw — the target stays, Writer is cleared
        void* Target = nullptr;                                                 // RGBA16F [H][TargetPitch], modified in place: scene colour or the bounding-volumes target
        int TargetPitch = 0;                                                    // pixels per row, 0 = W
        const float* SceneDepth = nullptr;                                      // float [H][DepthPitch]
        int DepthPitch = 0;
        uint32_t* Writer = nullptr;                                             // optional, [H][W]
        bool Blend = false;                                                     // UNLIT_BLEND_PSO
    };
    struct FTarget { void* Image = nullptr; int Pitch = 0; };                   // an RGBA16F image and its pixels per row (0 = W)
    // SceneRendering.cpp:1787-1819
    static FDrawParameters LightMeshes(void* Stream, const std::vector<vqhip_unlit_draw>* Draws, FTarget SceneColor, const float* SceneDepth, int DepthPitch = 0) {
        FDrawParameters p;
        p.Stream = Stream; p.Draws = Draws; p.Target = SceneColor.Image; p.TargetPitch = SceneColor.Pitch; p.SceneDepth = SceneDepth; p.DepthPitch = DepthPitch;
        p.Blend = false;
        return p;
    }
    // SceneRendering.cpp:1940-1989, the solid half
    static FDrawParameters LightBounds(void* Stream, const std::vector<vqhip_unlit_draw>* Draws, bool bReflectionsEnabled, FTarget SceneColor, FTarget BoundingVolumes,
                                       const float* SceneDepth, int DepthPitch = 0) {
        FDrawParameters p;
        const FTarget& t = bReflectionsEnabled ? BoundingVolumes : SceneColor;
        p.Stream = Stream; p.Draws = Draws; p.Target = t.Image; p.TargetPitch = t.Pitch; p.SceneDepth = SceneDepth; p.DepthPitch = DepthPitch;
        p.Blend = !bReflectionsEnabled;
        return p;
    }
    explicit UnlitDrawsPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { mWork.Release(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override { mWidth = Width; mHeight = Height; }
    void OnDestroyWindowSizeDependentResources() override { mWidth = mHeight = 0; }
    bool Reserve(uint64_t Triangles) { return mWork.Reserve(vqhip_unlit_draws_work_bytes(Triangles)); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !p->Target || !p->SceneDepth) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        uint64_t triangles = 0;
        const int numDraws = p->Draws ? (int)p->Draws->size() : 0;
        for (int d = 0; d < numDraws; ++d) triangles += (*p->Draws)[(size_t)d].mesh.numIndices / 3;
        if (!Reserve(triangles)) { mStatus = VQHIP_ERR_HIP; return; }
        vqhip_unlit_targets t = {};
        t.sceneColor = p->Target; t.pitch = p->TargetPitch; t.sceneDepth = p->SceneDepth; t.depth_pitch = p->DepthPitch; t.writer = p->Writer;
        mStatus = vqhip_unlit_draws(mCtx, p->Stream, numDraws ? p->Draws->data() : nullptr, numDraws, (int)mWidth, (int)mHeight, p->Blend ? 1 : 0, &t, mWork.ptr, mWork.bytes);
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }
    size_t GetWorkBytes() const { return mWork.bytes; }
private:
    WorkBuffer mWork;
    unsigned mWidth = 0, mHeight = 0;
};

// ---------------------------------------------------------------------------------------------------------------
// The line draws of VQRenderer::RenderSceneBoundingVolumes (SceneRendering.cpp:2286-2345): vqhip_line_draws at one sample per pixel (docs/DESIGN_DETAILS.md §7.24
// L1 .. L8). LineDrawsPass is what the two passes below share: the parameter block, the line count for the work size, the work buffer, the call. The target is
// the cleared Tex_SceneColorBoundingVolumes when reflections are on (the plane vqhip_composite_reflections blends) and scene colour when they are off (:507-511,
// :734-735); depth is the scene's (HipDepthPrePass's, one sample), tested LESS and never written; no blending. Writer is the library's addition. W and H are the
// window's. The MSAA PSOs are not built (§7.24).
// ---------------------------------------------------------------------------------------------------------------
class LineDrawsPass : public RenderPassBase {
public:
    struct FResourceParameters : public IRenderPassResourceCollection {};
    struct FDrawParameters : public IRenderPassDrawParameters {
        void* Stream = nullptr;
        const std::vector<vqhip_line_draw>* Draws = nullptr;                    // nullptr or empty: nothing to draw — the target stays, Writer is cleared
        void* Target = nullptr;                                                 // RGBA16F [H][TargetPitch], modified in place: scene colour or the bounding-volumes target
        int TargetPitch = 0;                                                    // pixels per row, 0 = W
        const float* SceneDepth = nullptr;                                      // float [H][DepthPitch]
        int DepthPitch = 0;
        uint32_t* Writer = nullptr;                                             // optional, [H][W]
    };
    struct FTarget { void* Image = nullptr; int Pitch = 0; };                   // an RGBA16F image and its pixels per row (0 = W)
    static uint64_t Lines(const vqhip_line_draw& d) {
        return d.kind == VQHIP_LINES_WIREFRAME ? (uint64_t)d.mesh.numIndices * d.numInstances : (uint64_t)d.mesh.numIndices * 3;
    }
    explicit LineDrawsPass(vqhip_ctx* Ctx) : RenderPassBase(Ctx) {}
    bool Initialize() override { return mCtx != nullptr; }
    void Destroy() override { mWork.Release(); }
    void OnCreateWindowSizeDependentResources(unsigned Width, unsigned Height, const IRenderPassResourceCollection* = nullptr) override { mWidth = Width; mHeight = Height; }
    void OnDestroyWindowSizeDependentResources() override { mWidth = mHeight = 0; }
    bool Reserve(uint64_t NumLines) { return mWork.Reserve(vqhip_line_draws_work_bytes(NumLines)); }
    void RecordCommands(const IRenderPassDrawParameters* pDrawParameters = nullptr) override {
        const FDrawParameters* p = static_cast<const FDrawParameters*>(pDrawParameters);
        if (!p || !p->Target || !p->SceneDepth) { mStatus = VQHIP_ERR_INVALID_ARG; return; }
        uint64_t lines = 0;
        const int numDraws = p->Draws ? (int)p->Draws->size() : 0;
        for (int d = 0; d < numDraws; ++d) lines += Lines((*p->Draws)[(size_t)d]);
        if (!Reserve(lines)) { mStatus = VQHIP_ERR_HIP; return; }
        vqhip_unlit_targets t = {};
        t.sceneColor = p->Target; t.pitch = p->TargetPitch; t.sceneDepth = p->SceneDepth; t.depth_pitch = p->DepthPitch; t.writer = p->Writer;
        mStatus = vqhip_line_draws(mCtx, p->Stream, numDraws ? p->Draws->data() : nullptr, numDraws, (int)mWidth, (int)mHeight, &t, mWork.ptr, mWork.bytes);
    }
    const void* GetWorkBuffer() const { return mWork.ptr; }
    size_t GetWorkBytes() const { return mWork.bytes; }
protected:
    static FDrawParameters Fill(void* Stream, const std::vector<vqhip_line_draw>* Draws, bool bReflectionsEnabled, FTarget SceneColor, FTarget BoundingVolumes,
                                const float* SceneDepth, int DepthPitch) {
        FDrawParameters p;
        const FTarget& t = bReflectionsEnabled ? BoundingVolumes : SceneColor;
        p.Stream = Stream; p.Draws = Draws; p.Target = t.Image; p.TargetPitch = t.Pitch; p.SceneDepth = SceneDepth; p.DepthPitch = DepthPitch;
        return p;
    }
private:
    WorkBuffer mWork;
    unsigned mWidth = 0, mHeight = 0;
};

// The WIREFRAME PSOs == VQRenderer::RenderBoundingBoxes (SceneRendering.cpp:1853-1922: one FInstancedWireframeRenderData is one draw; its cbuffer is the uploaded
// FFrameConstantBufferUnlitInstanced block, 512 matrices and then the colour) and the second half of VQRenderer::RenderLightBounds (:1991-2014: one FLightRenderData
// is one draw; its cbuffer is the uploaded FFrameConstantBufferUnlit block — the colour's alpha is NOT scaled by 0.01 in this loop).
class WireframePass : public LineDrawsPass {
public:
    // one batch of boxes: the cube, the instanced cbuffer on the device, the number of boxes in it (1 .. VQHIP_LINES_MAX_INSTANCES)
    static vqhip_line_draw Box(const vqhip_shadow_mesh& Cube, const void* InstancedCBuffer, uint32_t NumInstances) {
        vqhip_line_draw d = {};
        d.mesh = Cube; d.matModelViewProj = static_cast<const VQ_matrix*>(InstancedCBuffer);
        d.color = reinterpret_cast<const VQ_float4*>(static_cast<const VQ_matrix*>(InstancedCBuffer) + VQHIP_LINES_MAX_INSTANCES);
        d.numInstances = NumInstances; d.kind = VQHIP_LINES_WIREFRAME;
        return d;
    }
    // one light volume: the mesh and the cbuffer the solid half drew it with (a copy whose alpha is the render data's own)
    static vqhip_line_draw Bound(const vqhip_shadow_mesh& Mesh, const VQ_UnlitData* CBuffer) {
        vqhip_line_draw d = {};
        d.mesh = Mesh; d.matModelViewProj = &CBuffer->matModelViewProj; d.color = &CBuffer->color; d.numInstances = 1; d.kind = VQHIP_LINES_WIREFRAME;
        return d;
    }
    // SceneRendering.cpp:1853-1922
    static FDrawParameters BoundingBoxes(void* Stream, const std::vector<vqhip_line_draw>* Draws, bool bReflectionsEnabled, FTarget SceneColor, FTarget BoundingVolumes,
                                         const float* SceneDepth, int DepthPitch = 0) {
        return Fill(Stream, Draws, bReflectionsEnabled, SceneColor, BoundingVolumes, SceneDepth, DepthPitch);
    }
    // SceneRendering.cpp:1991-2014, the wire half
    static FDrawParameters LightBounds(void* Stream, const std::vector<vqhip_line_draw>* Draws, bool bReflectionsEnabled, FTarget SceneColor, FTarget BoundingVolumes,
                                       const float* SceneDepth, int DepthPitch = 0) {
        return Fill(Stream, Draws, bReflectionsEnabled, SceneColor, BoundingVolumes, SceneDepth, DepthPitch);
    }
    explicit WireframePass(vqhip_ctx* Ctx) : LineDrawsPass(Ctx) {}
};

// VQRenderer::RenderDebugVertexAxes (SceneRendering.cpp:2018-2058, DEBUGVERTEX_LOCALSPACEVECTORS_PSO): one MeshRenderData_t is one draw — the mesh's vertex buffer
// (position, normal, tangent at bytes 0, 12, 24) and index buffer as a POINT list, and the uploaded FObjectConstantBufferDebugVertexVectors block.
class VertexAxesPass : public LineDrawsPass {
public:
    static vqhip_line_draw Mesh(const vqhip_shadow_mesh& Mesh, const VQ_VertexAxesData* CBuffer) {
        vqhip_line_draw d = {};
        d.mesh = Mesh; d.axes = CBuffer; d.numInstances = 1; d.kind = VQHIP_LINES_VERTEX_AXES;
        return d;
    }
    static FDrawParameters VertexAxes(void* Stream, const std::vector<vqhip_line_draw>* Draws, bool bReflectionsEnabled, FTarget SceneColor, FTarget BoundingVolumes,
                                      const float* SceneDepth, int DepthPitch = 0) {
        return Fill(Stream, Draws, bReflectionsEnabled, SceneColor, BoundingVolumes, SceneDepth, DepthPitch);
    }
    explicit VertexAxesPass(vqhip_ctx* Ctx) : LineDrawsPass(Ctx) {}
};

} // namespace vqhip
