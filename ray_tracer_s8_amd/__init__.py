"""MI355X-native tile renderer for the ray-tracer-s8 slave hot path.

Product code: the HIP kernel + C-ABI (csrc/, include/rt_tile.h) and this thin host-side
mirror of the reference's RenderInfo/ImageSlice surface.  Nothing here imports oracle/.
"""
from ._abi import (BOUNCE_DTYPE, DIRECT_DTYPE, HIT_DTYPE, RAY_DTYPE, RT_BOUNCE_EMITTED, RT_BOUNCE_MISSED, RT_BOUNCE_SCATTERED, RT_FLAG_EXACT_SCAN, RT_FLAG_NO_BVH_CULL, RT_FLAG_NONE, RT_HIT_NONE, SPHERE_DTYPE,
                   TRIANGLE_DTYPE, AovPlanes, BounceRequest, Camera, DirectRequest, DenoiseRequest, NeeRequest, RT_GLOSSY_BOUNCE, RT_GLOSSY_MIS, RT_LIGHTS_AREA, RT_LIGHTS_CONE, RT_NEE_LIGHT_ONLY, RT_NEE_MIS, RtError, TileRequest, TileStats, TraceRequest, default_request)
from .interface import (Controller, FrameContext, ImageSlice, RenderInfo, RenderMeta, RenderSettings, Scene, Slave, World, aov_means,
                        denoise_scratch_bytes, init, render_frame_native)
from .film import Film
from .film_history import FilmHistory
from .film_sampler import FilmSampler
from .film_upsampler import FilmUpsampler
from .film_robust import FilmRobust
from .film_display import FilmDisplay
from .frame_encoder import FrameEncoder
from .film_bloom import FilmBloom

__all__ = [
    "NeeRequest", "RT_NEE_LIGHT_ONLY", "RT_NEE_MIS", "RT_LIGHTS_AREA", "RT_LIGHTS_CONE", "RT_GLOSSY_BOUNCE", "RT_GLOSSY_MIS", "DIRECT_DTYPE", "DirectRequest", "BOUNCE_DTYPE", "BounceRequest", "RT_BOUNCE_SCATTERED", "RT_BOUNCE_EMITTED", "RT_BOUNCE_MISSED",
    "HIT_DTYPE", "RAY_DTYPE", "RT_HIT_NONE", "RT_FLAG_EXACT_SCAN", "RT_FLAG_NO_BVH_CULL", "RT_FLAG_NONE", "SPHERE_DTYPE", "TRIANGLE_DTYPE", "RtError", "TileRequest", "TileStats",
    "TraceRequest", "AovPlanes", "Camera", "aov_means", "DenoiseRequest", "denoise_scratch_bytes", "default_request", "Controller", "FrameContext", "ImageSlice", "RenderInfo", "RenderMeta", "RenderSettings", "Scene", "Slave",
    "World", "init", "render_frame_native", "Film", "FilmHistory", "FilmSampler", "FilmUpsampler", "FilmRobust", "FilmDisplay", "FrameEncoder",
    "FilmBloom",
]
