// tests/compat_runtime: cv::KeyPoint lives in core.hpp of this stand-in (see README.md in this directory)
#pragma once
#include <opencv2/core/core.hpp>
