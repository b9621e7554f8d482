// oracle/cv_decl/opencv2/opencv.hpp -- CONTAINER DECLARATION ONLY, test infrastructure (read by oracle/ref_planner_probe.cpp
// and the reference sources it compiles in place, alone).
//
// The reference's DepthImagePlanner.hpp includes <opencv2/opencv.hpp>, which this image lacks.  The planner uses cv::Mat
// for three things, all in its constructor: .rows, .cols and .data (DepthImagePlanner.cpp:38-39, 61).  This header
// declares exactly those three fields and computes nothing: no pixel access, no arithmetic, no image operation.  Any
// pinned code path that used OpenCV beyond them would fail to COMPILE, so no number the probe writes can come from a
// stand-in for OpenCV.  (The reference also receives <algorithm> through OpenCV's includes; the recipe passes
// -include algorithm instead.)
#pragma once
namespace cv { struct Mat { int rows, cols; unsigned char *data; }; }
