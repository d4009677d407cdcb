// oracle/ref/matcher: cv::KeyPoint lives in core.hpp of the stand-in
#pragma once
#include <opencv2/core/core.hpp>
