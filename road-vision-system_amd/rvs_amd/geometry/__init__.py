from .projector import (CAM_PROJ_DTYPE, RV_CAM_PROJ_BYTES, GroundProjector, HomographyProjector,
                        build_camera_projectors, build_projector, find_homography,
                        pack_cam_table)

__all__ = ["GroundProjector", "HomographyProjector", "build_projector", "find_homography",
           "pack_cam_table", "build_camera_projectors", "CAM_PROJ_DTYPE", "RV_CAM_PROJ_BYTES"]
