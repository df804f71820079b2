// RtNative.cs — P/Invoke declarations of the MI355X trace library
// (include/rt_mi355.h) for the Unity reference project.  Drop into
// Assets/RayTracer/Native/ next to RayTracer.asmdef.
//
// SOURCE ONLY: there is no Mono/.NET/Unity in the build image, so this file
// is not compiled here.  tests/test_bindings.py checks that every DllImport
// names an entry point of the header and that every header entry point is
// declared here; the struct layouts follow the ctypes mirror
// (unity-raytracer_amd/abi.py) field for field, whose sizes/offsets
// tests/test_abi.py checks against the C header.
//
// RayTracer.asmdef:9 disallows `unsafe`, so no fixed buffers or pointers:
// arrays are pinned with GCHandle by the caller (RayTracingSetupNative.cs).
using System;
using System.Runtime.InteropServices;
using Unity.Mathematics;

namespace RayTracer.Native
{
    // MaterialData (MaterialData.cs:7-15) has a C# bool, which is not
    // blittable; the native form carries it as int32 (56 bytes).
    [StructLayout(LayoutKind.Sequential)]
    public struct RtMaterial
    {
        public float3 Diffuse, Ambient, Mirror, Specular;
        public float Phong;
        public int IsMirror;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtAabb { public float3 Min, Max; }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtMesh
    {
        public int FirstTriangle, TriangleCount;
        public RtMaterial Material;
        public RtAabb Aabb;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtSceneDesc
    {
        public IntPtr Triangles, TriangleNormals, TriangleMaterials;
        public int TriangleCount;
        public IntPtr MeshTriangles, MeshTriangleNormals;
        public int MeshTriangleTotal;
        public IntPtr Meshes;
        public int MeshCount;
        public IntPtr Spheres, SphereMaterials;
        public int SphereCount;
        public IntPtr PointLights;
        public int PointLightCount;
        public float3 AmbientRadiance;
    }

    // Row-major 4x4 (m[row * 4 + col]).  UnityEngine.Matrix4x4 stores its
    // elements column-major, so FromUnity transposes field by field.
    [StructLayout(LayoutKind.Sequential)]
    public struct RtMatrix
    {
        public float m00, m01, m02, m03, m10, m11, m12, m13, m20, m21, m22, m23, m30, m31, m32, m33;

        public static RtMatrix FromUnity(UnityEngine.Matrix4x4 m) => new RtMatrix
        {
            m00 = m.m00, m01 = m.m01, m02 = m.m02, m03 = m.m03,
            m10 = m.m10, m11 = m.m11, m12 = m.m12, m13 = m.m13,
            m20 = m.m20, m21 = m.m21, m22 = m.m22, m23 = m.m23,
            m30 = m.m30, m31 = m.m31, m32 = m.m32, m33 = m.m33,
        };
    }

    // One SceneMesh before extraction (SceneMesh.cs:11-53); 152 bytes.
    [StructLayout(LayoutKind.Sequential)]
    public struct RtMeshSource
    {
        public IntPtr Vertices;      // Vector3[] of Mesh.vertices, pinned
        public int VertexCount;
        public IntPtr Indices;       // int[] of Mesh.triangles, pinned
        public int IndexCount;
        public RtMatrix LocalToWorld;
        public RtMaterial Material;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtImagePlane
    {
        public int ResX, ResY;
        public float Distance, HalfH, HalfV;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtRenderParams
    {
        public float BgR, BgG, BgB, BgA;
        public int MaxBounces, Spp, BandIndex, BandCount, BandRows, Flags;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtStats
    {
        public ulong PrimaryRays, ShadowRays, ReflectionRays, BoxTests, TriangleTests, SphereTests, ShadingFetches;
        public double KernelMs, TotalMs;
        public ulong PrimarySceneMisses;
        public ulong ShadowRaysMoot;  // shadow rays whose answer cannot change the pixel (not traversed)
    }

    // rt_device_info: the GPUs one context drives (rt_create(N > 1)).
    [StructLayout(LayoutKind.Sequential)]
    public struct RtDeviceInfo
    {
        public int NumDevices, Gather;
        [MarshalAs(UnmanagedType.ByValArray, SizeConst = 16)] public int[] Devices;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtSceneInfo
    {
        public int Build, BvhWidth, Nodes, Primitives;
        public double BuildMs, TotalMs;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtBvhExportInfo
    {
        public int Nodes, TriangleRecords, SphereRecords, Reserved;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtRay { public float3 Origin, Direction; }

    [StructLayout(LayoutKind.Sequential)]
    public struct RtHit { public int Type, Index, MeshIndex; public float Distance; }

    public static class Rt
    {
        const string Lib = "rt_mi355";

        public const int OK = 0;
        public const int BuildSahHost = 0, BuildLbvhGpu = 1, BuildLbvhGpuBvh2 = 2, BuildSahRefit = 3;
        public const int FlagCountTests = 1, FlagWavefront = 2, FlagPacket = 4, FlagOutRgba8 = 8, FlagOutRgba16F = 16,
                         FlagAsync = 32, FlagRowOrder = 64, FlagNoCut = 256;

        [DllImport(Lib)] public static extern int rt_abi_version();
        public const int GatherNone = 0, GatherPeerCopy = 1, GatherRccl = 2;

        // numGpus > 1: one context renders every frame on GPUs 0..numGpus-1
        // (row bands, RCCL gather to GPU 0) — the same Color[] as one GPU.
        [DllImport(Lib)] public static extern int rt_create(out IntPtr ctx, int numGpus);
        [DllImport(Lib)] public static extern int rt_create_devices(out IntPtr ctx, [In] int[] devices, int numDevices,
                                                                   int gather);
        [DllImport(Lib)] public static extern int rt_get_device_info(IntPtr ctx, out RtDeviceInfo info);
        [DllImport(Lib)] public static extern void rt_destroy(IntPtr ctx);
        [DllImport(Lib)] public static extern IntPtr rt_last_error(IntPtr ctx);
        [DllImport(Lib)] public static extern int rt_set_stream(IntPtr ctx, IntPtr hipStream);
        [DllImport(Lib)] public static extern int rt_set_scene(IntPtr ctx, ref RtSceneDesc scene);
        [DllImport(Lib)] public static extern int rt_set_scene_ex(IntPtr ctx, ref RtSceneDesc scene, int build);
        [DllImport(Lib)] public static extern int rt_get_scene_info(IntPtr ctx, out RtSceneInfo info);
        // inspection: the 4-wide BVH as it lies in HBM (null arrays: counts only)
        [DllImport(Lib)] public static extern int rt_export_bvh(IntPtr ctx, [Out] byte[] nodes, [Out] byte[] triangleRecords,
                                                               [Out] byte[] sphereRecords, out RtBvhExportInfo info);
        [DllImport(Lib)] public static extern int rt_set_scene_source(IntPtr ctx, ref RtSceneDesc baseScene,
                                                                     [In] RtMeshSource[] meshes, int meshCount);
        [DllImport(Lib)] public static extern int rt_set_scene_source_ex(IntPtr ctx, ref RtSceneDesc baseScene,
                                                                        [In] RtMeshSource[] meshes, int meshCount,
                                                                        int build);
        [DllImport(Lib)] public static extern int rt_update_mesh_transforms(IntPtr ctx, [In] RtMatrix[] localToWorld,
                                                                           int meshCount);
        [DllImport(Lib)] public static extern int rt_render(IntPtr ctx, ref CameraData cam, ref RtImagePlane plane,
                                                           ref RtRenderParams p, [Out] UnityEngine.Color[] pixels,
                                                           out RtStats stats);
        // RGBA8 output straight into a Color32[] (Texture2D.SetPixels32 / LoadRawTextureData)
        [DllImport(Lib, EntryPoint = "rt_render")]
        public static extern int rt_render_rgba8(IntPtr ctx, ref CameraData cam, ref RtImagePlane plane,
                                                 ref RtRenderParams p, [Out] UnityEngine.Color32[] pixels,
                                                 out RtStats stats);
        [DllImport(Lib)] public static extern int rt_pixel_bytes(int flags);
        [DllImport(Lib)] public static extern int rt_finish(IntPtr ctx, out RtStats stats);
        [DllImport(Lib)] public static extern int rt_synchronize(IntPtr ctx);
        [DllImport(Lib)] public static extern int rt_render_device(IntPtr ctx, ref CameraData cam,
                                                                  ref RtImagePlane plane, ref RtRenderParams p,
                                                                  IntPtr devicePixels, UIntPtr outBytes,
                                                                  out RtStats stats);
        // frames in flight of one layout from their own cameras as one launch (device outputs back to back)
        [DllImport(Lib)] public static extern int rt_render_device_batch(IntPtr ctx, int numFrames,
                                                                        [In] CameraData[] cams, ref RtImagePlane plane,
                                                                        ref RtRenderParams p, IntPtr devicePixels,
                                                                        UIntPtr frameStrideBytes, out RtStats stats);
        [DllImport(Lib)] public static extern int rt_band_rows_local(int resolutionY, int bandIndex, int bandCount,
                                                                    int bandRows);
        [DllImport(Lib)] public static extern int rt_assemble_bands(IntPtr ctx, IntPtr gathered, int resolutionX,
                                                                   int resolutionY, int bandCount, int bandRows,
                                                                   IntPtr image);
        [DllImport(Lib)] public static extern int rt_assemble_bands_ex(IntPtr ctx, IntPtr gathered, int resolutionX,
                                                                      int resolutionY, int bandCount, int bandRows,
                                                                      int pixelBytes, IntPtr image);
        [DllImport(Lib)] public static extern int rt_intersect_rays(IntPtr ctx, [In] RtRay[] rays, int n,
                                                                   [Out] RtHit[] hits);
        // Device-resident ray queries: every pointer but ctx / p / stats is device memory on the
        // context's GPU; enqueued on the context's stream (rt_set_stream), nothing awaited.
        [DllImport(Lib)] public static extern int rt_intersect_rays_device(IntPtr ctx, IntPtr deviceRays, int n,
                                                                          IntPtr deviceHits);
        [DllImport(Lib)] public static extern int rt_occluded_rays_device(IntPtr ctx, IntPtr deviceRays,
                                                                         IntPtr deviceMaxDistanceSq, int n,
                                                                         IntPtr deviceOccluded);
        // stats: IntPtr.Zero (stream-ordered) or a pinned RtStats (the call then waits for the stream)
        [DllImport(Lib)] public static extern int rt_shade_rays_device(IntPtr ctx, IntPtr deviceRays, int n,
                                                                      ref RtRenderParams p, IntPtr deviceColors,
                                                                      UIntPtr outBytes, IntPtr stats);
        [DllImport(Lib)] public static extern float rt_spec_threshold();
        [DllImport(Lib)] public static extern int rt_debug_set(IntPtr ctx, int what, int value);  // tests only
        [DllImport(Lib)] public static extern int rt_debug_read(IntPtr ctx, int what, IntPtr output, long capacityBytes, out long bytesWritten);  // measuring builds only

        public static string LastError(IntPtr ctx) => Marshal.PtrToStringAnsi(rt_last_error(ctx));

        public static RtMaterial Material(MaterialData m) => new RtMaterial
        {
            Diffuse = m.DiffuseReflectance, Ambient = m.AmbientReflectance, Mirror = m.MirrorReflectance,
            Specular = m.SpecularReflectance, Phong = m.PhongExponent, IsMirror = m.IsMirror ? 1 : 0,
        };
    }
}
