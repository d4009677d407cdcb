// tests/compat_localba: the one member of Map the fragment touches
#pragma once
#include <mutex>
namespace ORB_SLAM2 {
class Map {
public:
    std::mutex mMutexMapUpdate;
};
}  // namespace ORB_SLAM2
