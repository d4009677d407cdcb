// oracle/ref/extractor: the reference includes this header for cv::resize, cv::copyMakeBorder and cv::GaussianBlur; the stand-in declares all of its cv:: in one file
#pragma once
#include "../../opencv2/core/core.hpp"
