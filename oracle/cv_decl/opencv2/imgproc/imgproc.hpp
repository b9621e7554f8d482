// oracle/cv_decl/opencv2/imgproc/imgproc.hpp -- CONTAINER DECLARATION ONLY, test infrastructure: the second OpenCV header
// DepthImagePlanner.hpp names.  It declares the same three-field cv::Mat as opencv2/opencv.hpp (see there) and computes
// nothing.
#pragma once
#include "../opencv.hpp"
