/* Declared double of <pcl/kdtree/kdtree_flann.h> -- NOT PCL.  The reference's scan registration includes the header and
 * uses nothing of it, so this is empty on purpose. */
#pragma once
