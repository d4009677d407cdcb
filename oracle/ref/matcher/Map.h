// oracle/ref/matcher: stand-in for the reference's include/Map.h (forced in with -include, guard defined so that the sibling the
// reference's MapPoint.h includes by quoted name expands to nothing).  Members: what src/MapPoint.cc touches.
#ifndef MAP_H
#define MAP_H
#include <mutex>
#include <set>
namespace ORB_SLAM2 {
class MapPoint;
class Map {
public:
    void EraseMapPoint(MapPoint *pMP) { erased.insert(pMP); }
    std::mutex mMutexPointCreation;
    std::set<MapPoint *> erased;      // read by nobody: the map keeps no list of points here
};
}  // namespace ORB_SLAM2
#endif
