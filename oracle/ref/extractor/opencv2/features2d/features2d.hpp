// oracle/ref/extractor: the reference includes this header for cv::FAST and cv::KeyPoint; the stand-in declares all of its cv:: in one file
#pragma once
#include "../../opencv2/core/core.hpp"
