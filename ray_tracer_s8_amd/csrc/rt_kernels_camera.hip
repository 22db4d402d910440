// Device code of the camera rays of a strip (rt_camera.hip.h): the tile's camera rays and the RNG states after them, one lane per
// (pixel, sample).  Its own translation unit: the tile, query, trace, AOV and denoiser kernels' code objects are untouched by it.
#include "rt_camera.hip.h"

namespace rtk {
CameraFn camera_rays_kernel(bool states) { return states ? rt_camera_rays_kernel<true> : rt_camera_rays_kernel<false>; }
}  // namespace rtk
