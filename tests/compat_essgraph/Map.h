// tests/compat_essgraph: the members of Map the function touches
#pragma once
#include <mutex>
#include <vector>
namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint;
class Map {
public:
    std::vector<KeyFrame *> GetAllKeyFrames() { return mvpKeyFrames; }
    std::vector<MapPoint *> GetAllMapPoints() { return mvpMapPoints; }
    long unsigned int GetMaxKFid() { return mnMaxKFid; }
    std::vector<KeyFrame *> mvpKeyFrames;
    std::vector<MapPoint *> mvpMapPoints;
    long unsigned int mnMaxKFid = 0;
    std::mutex mMutexMapUpdate;
};
}  // namespace ORB_SLAM2
